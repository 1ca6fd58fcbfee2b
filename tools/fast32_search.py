"""Directed worst-case search for the float32 fast path's clipped mean (tools/fast32_model.py) -> tests/golden/g14_fast32_columns.npz.

Hill-climbs, per frame count, on the model's PRE-ROUNDING error |cf + ms32 - mean| in ulps of the mean (the rounded result
only moves in whole ulps and gives a climb nothing to follow), over columns the fast path accepts under a given mean guard:
  (a) guard 16 (release, rms(d) <= |c| / 4): the accepted columns with the largest error - the suite's stress columns;
  (b) guard 4 (the old rms(d) <= |c| / 2): accepted columns whose rounded mean is >= 2 ulp from the correctly rounded one -
      on a release build these must take the exact path (the model checks that they fail guard 16).
Both forms of the fast path (tools/fast32_model.py): 'calib' (tails of 4: the fused-calibration fast kernel, the complete
kernel) -> arrays a_N / b_N, and 'plain' (tails of 8: the fast kernel without calibration) -> ap_N / bp_N.  The 129..512-frame
chunk path is not modelled and not searched.
Starting columns are biased to the weak spots: means just below a power of two (where ulp / |m| is smallest), both signs,
skewed shapes (two-level, exponential) and rms(d) / |c| packed against the guard's edge.  Seeded: the fixture is reproducible.

    python tools/fast32_search.py            # search, write the fixture, print the worst error per N
    python tools/fast32_search.py --check    # search again and compare with the committed fixture byte for byte
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast32_model as fm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g14_fast32_columns.npz')
FRAME_COUNTS = (16, 24, 32, 48, 64, 96, 128, 13, 30, 61)
KEEP = 24                   # columns per N and fixture part
POP, GENS = 6000, 24        # candidates per generation, generations


def _shape(rng, kind, M, N):
    """[M, N] deviations with median 0 and rms 1 about it, of the given shape."""
    if kind == 0:
        z = rng.normal(size=(M, N))
    elif kind == 1:                                          # two levels, a minority of the values at the upper one
        k = rng.integers(1, max(2, N // 3), M)
        z = (np.arange(N)[None, :] < k[:, None]).astype(np.float64)
        z = rng.permuted(z, axis=1) + 1e-3 * rng.normal(size=(M, N))
    elif kind == 2:
        z = rng.exponential(size=(M, N))
    else:
        z = rng.uniform(-1, 1, (M, N))
    z = z * np.where(rng.random(M) < 0.5, 1.0, -1.0)[:, None]       # skew to either side
    z = z - np.median(z, axis=1, keepdims=True)
    return z / np.maximum(np.sqrt((z * z).mean(axis=1, keepdims=True)), 1e-30)


def _fresh(rng, M, N, guard):
    edge = 1.0 / np.sqrt(guard)                              # rms(d) / |c| at the guard's edge
    r = edge * rng.uniform(0.7, 1.0, M)
    z = np.concatenate([_shape(rng, kind, M // 4 + (kind < M % 4), N) for kind in range(4)])[:M]
    z = z[rng.permutation(M)]
    # the column's mean just below a power of two, either sign
    target = np.ldexp(1.0 - rng.uniform(0, 2.0 ** -10, M), rng.integers(-6, 14, M)) * np.where(rng.random(M) < 0.5, 1.0, -1.0)
    c = target / (1.0 + r * z.mean(axis=1))
    return (c[:, None] * (1.0 + r[:, None] * z)).astype(np.float32)


def _mutate(rng, cols):
    M, N = cols.shape
    out = cols.astype(np.float64).copy()
    kind = rng.integers(0, 3, M)
    s = kind == 0                                            # scale the whole column (moves the mean against the binade)
    out[s] *= 1.0 + rng.normal(0, 2.0 ** -16, s.sum())[:, None]
    s = kind == 1                                            # a few values nudged by a few ulp .. 1e-4 relative
    j = rng.integers(0, N, (M, 3))
    for k in range(3):
        rel = rng.normal(0, 1, M) * 10.0 ** rng.uniform(-7, -4, M)
        out[np.arange(M)[s], j[s, k]] *= 1.0 + rel[s]
    s = kind == 2                                            # one value moved towards or away from the median
    jj = rng.integers(0, N, M)
    med = np.median(out, axis=1)
    f = rng.uniform(-0.05, 0.05, M)
    rows = np.arange(M)[s]
    out[rows, jj[s]] += f[s] * (out[rows, jj[s]] - med[s])
    return out.astype(np.float32)


def search(N, guard, seed, mean_check=True, form='calib'):
    """-> (columns [KEEP, N] float32, their pre-rounding errors) - the accepted columns with the largest error."""
    rng = np.random.default_rng(seed)
    best = np.zeros((0, N), np.float32)
    for g in range(GENS):
        fresh = _fresh(rng, POP // 2 if g else POP, N, guard)
        kids = _mutate(rng, np.repeat(best, max(1, (POP // 2) // max(len(best), 1)), axis=0)) if len(best) else best
        cand = np.concatenate([best, kids, fresh])
        e = fm.evaluate(cand, guard=guard, mean_check=mean_check, form=form)
        score = np.where(e['done'] & np.isfinite(e['err_ulp']), np.abs(e['err_ulp']), -1.0)
        order = np.argsort(-score, kind='stable')
        order = order[score[order] >= 0][:4 * KEEP]
        # distinct columns only
        _, first = np.unique(cand[order], axis=0, return_index=True)
        order = order[np.sort(first)]
        best = cand[order]
    e = fm.evaluate(best, guard=guard, mean_check=mean_check, form=form)
    return best, e


def build():
    arrays = {}
    report = []
    for form, key, seed in (('calib', '', 0), ('plain', 'p', 5000)):
        for N in FRAME_COUNTS:
            a, ea = search(N, fm.GUARD_RELEASE, seed + 1400 + N, form=form)
            a, erra = a[:KEEP], ea['err_ulp'][:KEEP]
            b, eb = search(N, fm.GUARD_OLD, seed + 2400 + N, form=form)
            sel = (eb['ulp_dist'] >= 2) & eb['done']
            b = b[sel][:KEEP]
            arrays['a%s_%d' % (key, N)] = a
            arrays['a%s_err_%d' % (key, N)] = erra.astype(np.float64)
            arrays['b%s_%d' % (key, N)] = b
            report.append((form, N, float(np.abs(erra).max()), int(sel.sum()), float(np.abs(eb['err_ulp']).max()), int(fm.exact_model(N))))
    return arrays, report


def to_bytes(arrays):
    """An .npz archive, members stored uncompressed with fixed timestamps (np.savez stamps the current time, and deflate's
    output depends on the zlib build): the same arrays, the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', compression=zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            m = io.BytesIO()
            np.lib.format.write_array(m, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_STORED
            info.external_attr = 0o644 << 16
            z.writestr(info, m.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='regenerate and compare with the committed fixture')
    ap.add_argument('--out', default=FIXTURE)
    args = ap.parse_args()
    arrays, report = build()
    print(' form    N  worst |err| guard 16 (ulp)  >=2-ulp columns guard 4  worst |err| guard 4  model bit-exact')
    for form, N, ea, nb, eb, ex in report:
        print('%5s %4d  %26.4f  %23d  %19.4f  %15s' % (form, N, ea, nb, eb, 'yes' if ex else 'no'))
    data = to_bytes(arrays)
    if args.check:
        with open(args.out, 'rb') as f:
            same = f.read() == data
        print('fixture %s: %s' % (args.out, 'identical' if same else 'DIFFERS'))
        return 0 if same else 1
    with open(args.out, 'wb') as f:
        f.write(data)
    print('wrote %s (%d bytes)' % (args.out, len(data)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
