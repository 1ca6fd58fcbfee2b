#!/opt/conda/bin/python3.9 -B
"""Golden group G15: the per-box statistics photutils' Background2D takes from astropy, computed by astropy itself.

RUN ONLY IN THE BUILD CONTAINER:   /opt/conda/bin/python3.9 -B tests/golden/make_golden_boxstats.py

photutils is absent, astropy (4.3.1) is not.  What Background2D does with its boxes is, per its published source:
    box_data [nboxes, box_h * box_w], the input mask, the 'pad' edge pixels and non-finite pixels as NaN
    clipped  = SigmaClip(sigma, maxiters)(box_data, axis=1, masked=False)      (default cenfunc 'median', stdfunc 'std')
    nmasked0 = count of NaN in box_data; nfinal = count of non-NaN in clipped
    median   = np.nanmedian(clipped, axis=1)    (MedianBackground);   std = np.nanstd(clipped, axis=1)   (StdBackgroundRMS)
With an axis and the string cenfunc / stdfunc, SigmaClip.__call__ takes astropy's compiled path (_sigmaclip_fast): the box is
converted to float64, the bounds come from the C loop on a compacted buffer, and the returned array masks what lies outside the
LAST bounds - so a value that an earlier, tighter pass removed can come back.  SigmaClip stores `maxiters or np.inf`:
maxiters=0 means "clip until nothing changes", not "do not clip".
This script runs exactly those calls and records inputs and outputs (tests/test_oracle_golden.py holds
oracle/background_ref.box_clipped_stats to them, tests/test_gpu_boxstats_golden.py the HIP kernel), plus
    std_hp   a float64 standard deviation of the same survivors from math.fsum (exactly rounded sums): the high-precision value
    history  a float64 restatement of the C loop (sequential sums, as compute_bounds.c) whose final bounds are asserted equal to
             the bounds astropy returns (to 1e-12, the rounding of the compiled sums) and its survivor count to astropy's; it supplies what astropy does not expose - per iteration the upper middle element of
             the survivors and the bounds - for the coverage conditions asserted at the end of main():
      (a) in >= 3 boxes of more than 32768 pixels the leading 11 bits of the upper middle element's order-preserving float32 key
          change between consecutive iterations;
      (b) in >= 1 box the survivors of the final bounds differ from the survivors of the running intersection of all bounds;
      (c) even-count boxes exist whose two middle survivors are equal, differ inside one 10-bit bin (same leading 22 key bits),
          and differ in their leading 22 key bits.
Images are stored in the archive (integer-valued ones as integers times a power-of-two scale, exceptional values - NaN, +-inf,
-0.0 - as an index / value list): nothing depends on a random stream being the same under two interpreters.
"""
import json
import math
import os
import sys
import warnings

warnings.filterwarnings('ignore')
import numpy as np

for nm, fn in [('asscalar', lambda a: a.item()), ('alen', len), ('msort', lambda a: np.sort(a, axis=0)),
               ('product', np.prod), ('cumproduct', np.cumprod), ('sometrue', np.any), ('alltrue', np.all),
               ('float', float), ('int', int), ('bool', bool), ('object', object), ('complex', complex), ('str', str)]:
    if not hasattr(np, nm):
        setattr(np, nm, fn)
import astropy
import astropy.stats.sigma_clipping as sc
sc.HAS_BOTTLENECK = False
from astropy.stats import SigmaClip

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_PIXELS = 32768                  # boxes above this many pixels are not staged on chip by the kernel ("non-resident")
SIZE_LIMIT = 1018854                # the largest fixture committed before G15 (g11_calibrate_f64_cases.npz)


def f32_key(x):
    """Order-preserving uint32 key of float32 values (the radix-select key)."""
    u = np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32).astype(np.int64)
    k = np.where(u & 0x80000000, 0xffffffff - u, u | 0x80000000)
    return k if np.ndim(x) else k[0]


def box_rows(img, mask, bh, bw):
    """Background2D's box_data: [ny * nx, bh * bw] float32, NaN = masked / padded / non-finite."""
    H, W = img.shape
    ny, nx = -(-H // bh), -(-W // bw)
    pad = np.full((ny * bh, nx * bw), np.nan, np.float32)
    pad[:H, :W] = np.where(np.isfinite(img), img, np.nan)
    if mask is not None:
        m = np.zeros(pad.shape, bool)
        m[:H, :W] = mask != 0
        pad[m] = np.nan
    return pad.reshape(ny, bh, nx, bw).transpose(0, 2, 1, 3).reshape(ny * nx, bh * bw), ny, nx


def seqsum(a):
    return float(np.cumsum(a)[-1]) if a.size else 0.0


cov_all_clipped = []


def history(values, sigma, maxiters):
    """The loop of astropy's compute_bounds.c on one box, float64, sequential sums: list of (upper middle element, lower
    middle element, count, lo, hi) per iteration, the final bounds, and the running intersection of all bounds."""
    buf = values[np.isfinite(values)].astype(np.float64)
    hist = []
    lo = hi = np.nan
    lo_run, hi_run = -np.inf, np.inf
    it = 0
    while buf.size:
        n = buf.size
        s = np.sort(buf)
        up, low = s[n // 2], s[(n - 1) // 2]
        median = up if n % 2 else 0.5 * (low + up)
        mean = seqsum(buf) / n
        std = math.sqrt(seqsum((mean - buf) ** 2) / n)
        lo, hi = median - sigma * std, median + sigma * std
        lo_run, hi_run = max(lo_run, lo), min(hi_run, hi)
        hist.append((up, low, n, lo, hi))
        new = buf[(buf >= lo) & (buf <= hi)]
        if new.size == n:
            break
        buf = new
        it += 1
        if maxiters and it >= maxiters:
            break
        if buf.size == 0:
            # a pass that removes EVERYTHING before maxiters is reached: the next pass divides 0 by 0, the bounds are NaN, no
            # comparison with them masks anything, and every finite value of the box survives
            lo = hi = np.nan
            cov_all_clipped.append(1)
            break
    return hist, lo, hi, lo_run, hi_run


def record(out, meta, cov, name, img_key, img, mask_key, mask, bh, bw, sigma, maxiters):
    rows, ny, nx = box_rows(img, mask, bh, bw)
    clip = SigmaClip(sigma=sigma, maxiters=maxiters)
    clipped, blo, bhi = clip(rows, axis=1, masked=False, return_bounds=True)
    assert clipped.shape == rows.shape
    median = np.nanmedian(clipped, axis=1)
    std = np.nanstd(clipped, axis=1)
    nfin = np.count_nonzero(~np.isnan(clipped), axis=1)
    nm0 = np.count_nonzero(np.isnan(rows), axis=1)
    std_hp = np.full(len(rows), np.nan)
    nb = len(rows)
    up_hist = np.full((nb, 12), np.nan, np.float32)
    for b in range(nb):
        surv = clipped[b][~np.isnan(clipped[b])]
        if surv.size:
            v = [float(x) for x in surv]
            mean = math.fsum(v) / len(v)                       # (exactly rounded sum) / n
            std_hp[b] = math.sqrt(math.fsum((x - mean) ** 2 for x in v) / len(v))
        hist, lo, hi, lo_run, hi_run = history(rows[b], sigma, maxiters)
        if not hist:
            assert np.isnan(blo[b]) and np.isnan(bhi[b]) and nfin[b] == 0
            continue
        # the restated loop IS astropy's loop, up to the rounding of its compiled sums: same bounds, same survivors
        tol = 1e-12 * max(abs(lo), abs(hi))
        assert (np.isnan(lo) and np.isnan(blo[b]) and np.isnan(bhi[b])) or (abs(lo - blo[b]) <= tol and abs(hi - bhi[b]) <= tol), (name, b, lo, blo[b], hi, bhi[b])
        x = rows[b][np.isfinite(rows[b])].astype(np.float64)
        final = ~((x < lo) | (x > hi))
        running = (x >= lo_run) & (x <= hi_run)
        assert final.sum() == nfin[b]
        if np.isnan(lo):
            cov['nanbounds'].append((name, b))
            continue
        for i, h in enumerate(hist[:12]):
            up_hist[b, i] = h[0]
        # coverage bookkeeping
        keys = f32_key(np.array([h[0] for h in hist], np.float32)) >> 21
        if bh * bw > LDS_PIXELS and np.any(keys[1:] != keys[:-1]):
            cov['a'].append((name, b, [int(k) for k in keys]))
        if final.sum() != running.sum():
            cov['b'].append((name, b, int(final.sum()), int(running.sum())))
        s = np.sort(x[final])
        if s.size and s.size % 2 == 0:
            k1, k2 = int(f32_key(np.float32(s[s.size // 2 - 1]))), int(f32_key(np.float32(s[s.size // 2])))
            cov['c_equal' if k1 == k2 else 'c_same22' if (k1 >> 10) == (k2 >> 10) else 'c_cross22'].append((name, b))
        cov['odd' if s.size % 2 else 'even'].append((name, b))
    k = len(meta)
    out[f'c{k}_median'] = median.reshape(ny, nx)
    out[f'c{k}_std'] = std.reshape(ny, nx)
    out[f'c{k}_std_hp'] = std_hp.reshape(ny, nx)
    out[f'c{k}_count'] = nfin.reshape(ny, nx).astype(np.int64)
    out[f'c{k}_nmasked0'] = nm0.reshape(ny, nx).astype(np.int64)
    out[f'c{k}_lo'] = np.asarray(blo, np.float64).reshape(ny, nx)
    out[f'c{k}_hi'] = np.asarray(bhi, np.float64).reshape(ny, nx)
    out[f'c{k}_upper_middle'] = up_hist.reshape(ny, nx, 12)
    assert clipped.dtype == median.dtype == std.dtype == np.float64
    meta.append(dict(case=k, name=name, image=img_key, mask=mask_key, box=[bh, bw], sigma=sigma, maxiters=maxiters,
                     mesh=[ny, nx], dtype=str(median.dtype),
                     form='256-resident' if bh * bw <= 8192 else '1024-resident' if bh * bw <= LDS_PIXELS else '1024-non-resident'))


def store_image(out, key, img, scale=None):
    """float32 image `img`; with `scale` (a power of two) the ordinary values are integers times scale and are stored as
    integers, NaN / +-inf / -0.0 in an (index, value) list.  decode: see tests/util.py:g15_image."""
    img = np.asarray(img, np.float32)
    if scale is None:
        out[key] = img
        return
    special = ~np.isfinite(img) | ((img == 0) & np.signbit(img))
    q = np.where(special, 0, img.astype(np.float64) / scale)
    qi = np.rint(q).astype(np.int64)
    assert np.array_equal(qi, q)
    dt = np.int16 if np.abs(qi).max() < 32768 else np.int32
    out[key] = qi.astype(dt)
    out[key + '_scale'] = np.float64(scale)
    out[key + '_special_idx'] = np.flatnonzero(special).astype(np.int64)
    out[key + '_special_val'] = img.ravel()[special.ravel()]
    back = (out[key].astype(np.float64) * scale).astype(np.float32)
    back.ravel()[out[key + '_special_idx']] = out[key + '_special_val']
    assert np.array_equal(back.view(np.uint32), img.view(np.uint32))


def stars(rng, img, n, amp=(100, 20000)):
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(n):
        cy, cx, a, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(*amp), rng.uniform(1.2, 2.5)
        r = int(6 * s) + 2
        y0, y1, x0, x1 = max(0, int(cy) - r), min(H, int(cy) + r), max(0, int(cx) - r), min(W, int(cx) + r)
        img[y0:y1, x0:x1] += a * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * s * s))


def save(name, out, meta):
    out['_meta'] = np.array(json.dumps(meta))
    out['_versions'] = np.array(json.dumps(dict(astropy=astropy.__version__, numpy=np.__version__, python=sys.version.split()[0],
                                                 bottleneck='disabled', photutils='absent: Background2D box steps restated '
                                                 'with its own third-party calls (SigmaClip, np.nanmedian, np.nanstd)')))
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < SIZE_LIMIT, (name, size)
    print('wrote', name, len(meta), 'cases', size, 'bytes')


# (box_h, box_w) per launch form of the kernel on the 400 x 420 images: 7 x 6, 4 x 4 and 3 x 3 meshes, last row / column ragged
BOX_SMALL, BOX_MID, BOX_BIG = (64, 70), (110, 120), (182, 184)


def main():
    cov = dict(nanbounds=[], a=[], b=[], c_equal=[], c_same22=[], c_cross22=[], odd=[], even=[])
    H, W = 400, 420
    yy, xx = np.mgrid[0:H, 0:W]

    # ---- file A: integer-valued raw-frame data (heavy ties), constant data, one survivor, fully masked boxes ----
    out, meta = {}, []
    rng = np.random.default_rng(1501)
    raw = rng.poisson(36.0, (H, W)).astype(np.float64) + 264.0 + np.floor(0.02 * xx + 0.015 * yy)
    stars(rng, raw, 120)
    raw = np.clip(np.rint(raw), 0, 65535).astype(np.float32)
    store_image(out, 'img_raw', raw, 1.0)
    mask3 = (rng.random((H, W)) < 0.03).astype(np.uint8)
    mask3[150:200, 100:260] = 1
    out['mask_3pct'] = mask3
    for box in (BOX_SMALL, BOX_MID, BOX_BIG):
        for sigma, maxiters in ((3.0, 5), (2.0, 10), (0.5, 0), (3.0, 1)):
            record(out, meta, cov, 'raw', 'img_raw', raw, 'mask_3pct', mask3, box[0], box[1], sigma, maxiters)
    record(out, meta, cov, 'raw-nomask', 'img_raw', raw, None, None, BOX_BIG[0], BOX_BIG[1], 3.0, 5)
    # two-level and constant data: box columns < 210 hold 5 / 9 in equal numbers around a ragged pattern, the rest 7.25
    flat = np.full((H, W), 7.25, np.float32)
    flat[:, :210] = np.where((yy[:, :210] + xx[:, :210]) % 2 == 0, 5.0, 9.0)
    flat[300:, 300:] = np.where((yy[300:, 300:] // 3 + xx[300:, 300:]) % 2 == 0, 7.25, np.float32(7.2500005))
    store_image(out, 'img_flat', flat)
    mflat = np.zeros((H, W), np.uint8)
    mflat[0:182, 0:184] = 1                                      # fully masked boxes in every form
    mflat[182:364, 184:368] = 1
    mflat[200, 200] = 0                                          # one unmasked pixel in its box in every form
    mflat[:, 419] = 1
    mflat[399, 7] = 1                                            # odd / even survivor counts in the ragged boxes
    out['mask_flat'] = mflat
    for box in (BOX_SMALL, BOX_MID, BOX_BIG):
        for sigma, maxiters in ((3.0, 5), (0.5, 10), (2.0, 0)):
            record(out, meta, cov, 'flat', 'img_flat', flat, 'mask_flat', mflat, box[0], box[1], sigma, maxiters)
    save('g15_boxstats_a.npz', out, meta)

    # ---- file B: background-subtracted sky (both signs, +-0.0, NaN / +-inf), quantised to 1 / 64 ----
    out, meta = {}, []
    rng = np.random.default_rng(1502)
    zero = rng.normal(0.0, 6.0, (H, W)) + 0.9 * np.sin(xx / 97.0) * np.cos(yy / 71.0) + 0.35
    stars(rng, zero, 260, amp=(30, 20000))
    zero = (np.rint(zero * 64.0) / 64.0).astype(np.float32)
    zero[rng.integers(0, H, 300), rng.integers(0, W, 300)] = -0.0
    zero[rng.integers(0, H, 300), rng.integers(0, W, 300)] = 0.0
    zero[rng.integers(0, H, 40), rng.integers(0, W, 40)] = np.nan
    zero[rng.integers(0, H, 40), rng.integers(0, W, 40)] = np.inf
    zero[rng.integers(0, H, 40), rng.integers(0, W, 40)] = -np.inf
    zero[260:270, 300:330] = np.inf
    store_image(out, 'img_zero', zero, 1.0 / 64.0)
    mask2 = (rng.random((H, W)) < 0.02).astype(np.uint8)
    mask2[364:, 368:] = 1                                        # the ragged corner box of the 3 x 3 mesh: fully masked
    out['mask_2pct'] = mask2
    for box in (BOX_SMALL, BOX_MID, BOX_BIG):
        for sigma, maxiters in ((3.0, 5), (2.0, 10), (3.0, 10), (0.5, 5), (2.0, 1), (3.0, 0)):
            record(out, meta, cov, 'zero', 'img_zero', zero, 'mask_2pct', mask2, box[0], box[1], sigma, maxiters)
    record(out, meta, cov, 'zero-nomask', 'img_zero', zero, None, None, BOX_BIG[0], BOX_BIG[1], 2.0, 5)
    save('g15_boxstats_b.npz', out, meta)

    # ---- file C: continuous float32 data: sky near zero and at a negative level (small images, every clip setting),
    #      and searched boxes in which the last bounds re-admit what an earlier pass removed ----
    out, meta = {}, []
    rng = np.random.default_rng(1503)
    h, w = 150, 170
    y2, x2 = np.mgrid[0:h, 0:w]
    near0 = rng.normal(0.1, 6.0, (h, w)) + 0.004 * x2 - 0.003 * y2
    stars(rng, near0, 40)
    near0 = near0.astype(np.float32)
    near0[3, 5] = np.nan
    near0[70:74, 80:90] = -np.inf
    near0[10, 10], near0[10, 11] = 0.0, -0.0
    store_image(out, 'img_near0', near0)
    neg = rng.normal(-1000.37, 6.0, (h, w))
    stars(rng, neg, 40)
    neg[rng.random((h, w)) < 0.01] -= 300.0                      # low outliers too
    neg = neg.astype(np.float32)
    store_image(out, 'img_neg', neg)
    mask5 = (rng.random((h, w)) < 0.05).astype(np.uint8)
    out['mask_5pct'] = mask5
    for sigma in (0.5, 2.0, 3.0):
        for maxiters in (0, 1, 5, 10):
            record(out, meta, cov, 'near0', 'img_near0', near0, 'mask_5pct', mask5, 40, 45, sigma, maxiters)
            record(out, meta, cov, 'neg', 'img_neg', neg, 'mask_5pct', mask5, 40, 45, sigma, maxiters)
    record(out, meta, cov, 'neg-mid', 'img_neg', neg, 'mask_5pct', mask5, 100, 100, 3.0, 5)
    record(out, meta, cov, 'near0-mid', 'img_near0', near0, None, None, 100, 100, 2.0, 10)
    record(out, meta, cov, 'neg-whole', 'img_neg', neg, 'mask_5pct', mask5, 150, 170, 2.0, 5)
    # coverage (b): search small images whose boxes change survivors when the last bounds are applied to all the data
    found = 0
    for seed in range(4000):
        r = np.random.default_rng(150300 + seed)
        kind = seed % 3
        hh, ww = 48, 60
        if kind == 0:
            im = np.concatenate([r.normal(0, 1, 1700), r.normal(r.uniform(1.5, 4), r.uniform(0.3, 1.5), 1180)])
        elif kind == 1:
            im = r.exponential(1.0, hh * ww) * r.choice([1.0, -1.0], hh * ww, p=[0.8, 0.2])
        else:
            im = np.rint(r.gamma(2.0, 3.0, hh * ww))
        im = r.permutation(im).reshape(hh, ww).astype(np.float32)
        hit = False
        for sigma, maxiters in ((0.5, 5), (0.5, 10), (2.0, 5)):
            rows, _, _ = box_rows(im, None, 16, 20)
            for b in range(len(rows)):
                _, lo, hi, lo_run, hi_run = history(rows[b], sigma, maxiters)
                x = rows[b][np.isfinite(rows[b])].astype(np.float64)
                if not np.isnan(lo) and ((x >= lo) & (x <= hi)).sum() != ((x >= lo_run) & (x <= hi_run)).sum():
                    hit = True
            if hit:
                store_image(out, f'img_readmit{found}', im)
                record(out, meta, cov, f'readmit{found}', f'img_readmit{found}', im, None, None, 16, 20, sigma, maxiters)
                found += 1
                break
        if found >= 4:
            break
    save('g15_boxstats_c.npz', out, meta)

    # ---- coverage conditions, from what was recorded above ----
    print('coverage (a): %d non-resident boxes change the 11-bit prefix between iterations' % len(cov['a']))
    for c in cov['a'][:6]:
        print('   ', c)
    print('coverage (b): %d boxes where the last bounds re-admit / differ from the running intersection' % len(cov['b']), cov['b'][:6])
    print('coverage (c): equal %d, same 22-bit prefix %d, different 22-bit prefix %d; odd %d even %d survivor counts'
          % (len(cov['c_equal']), len(cov['c_same22']), len(cov['c_cross22']), len(cov['odd']), len(cov['even'])))
    assert len(set((n, b) for n, b, _ in cov['a'])) >= 3, 'coverage (a)'
    assert len(cov['b']) >= 1, 'coverage (b)'
    assert cov['c_equal'] and cov['c_same22'] and cov['c_cross22'], 'coverage (c)'
    assert cov['odd'] and cov['even']
    print('boxes emptied by a pass before maxiters (NaN bounds, every finite value survives): %d' % len(cov['nanbounds']), cov['nanbounds'][:4])
    assert cov['nanbounds']


if __name__ == '__main__':
    main()
