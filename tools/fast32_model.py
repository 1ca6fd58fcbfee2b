"""Host model of the float32 fast path's clipped mean (clip_fast32 in astrophotography_amd/csrc/stack_reduce.h and the
outputs of its callers: mean = cf + ms32).  NumPy, CPU only; vectorised over columns.

Reproduces in float32, operation by operation and in the kernel's association:
  - the core sums over mirror pairs (i, NP-1-i), i in [T, NP/2), in four chains by i & 3, Sc = (S0 + S1) + (S2 + S3) - the
    packed form (two v2f chains, NP <= 120: Sp0 = chains 0 / 1, Sp1 = chains 2 / 3) and the scalar 4-chain form (NP = 128,
    the complete kernel's MODE 0) add the same terms in the same order, so one model serves both;
  - the tail tables SL / SH (and QL / QH), summed from the inside out;
  - the padded slot counts: plo = (NP - N) // 2 -inf pads below, phi = NP - N - plo +inf pads above;
  - the clip passes with their sure / unsure margins (rho), trims of up to T per side, the final re-admission test;
  - the range guard and the mean-accuracy guard G Q <= n c^2 (APGPU_FAST32_MEAN_GUARD, 16 in release builds);
  - the mean: y = rcp(n), q0 = S y, ms32 = fma(fma(-n, q0, S), y, q0), mean = cf + ms32, and above 96 slots the
    a-posteriori test of finish_fast_column (stack_kernels.h) on it.

Two FORMS, by tail length T (what the clip can trim per side; the core sums start at T, so T sets the association):
  - 'calib': T = kFastTail = 4 for full columns, fast_tail_padded (6 / 8) for padded ones - stack_fast_kernel with the fused
    calibration (MODE 1, the benchmark's kernel) and the complete kernel's fast branch (reduce_and_store, MODE 0);
  - 'plain': T = 8 (6 below 20 slots) - stack_fast_kernel on stacks without the fused calibration (MODE 2: longer tails hold
    the lane's non-finite values), the PLUS planes included.  For finite columns MODE 2's per-lane cursors equal the pads.
A column fed in ascending order leaves the sorting networks unchanged (every compare-exchange lists its wires in ascending
order), so for such input the model's order is the kernel's.  Not modelled: the 129..512-frame chunk path (stack_chunks.hip),
whose sums run over chunk partials in another association.

Exactness: every float32 addition / multiplication is NumPy's (correctly rounded), fma is emulated exactly (fma32).  The one
operation not reproduced is the hardware reciprocal v_rcp_f32 (about 1 ulp): the model uses the correctly rounded 1 / n.  For n
a power of two both are exact, so the model is BIT-EXACT there (tests/test_gpu_fast32_mean.py pins the kernels to it); for other
n it is a search aid only (the mean may differ from the kernel's in the last bit).  Nothing here runs on a GPU.
"""
import numpy as np

F32 = np.float32
RHO = F32(2.0 ** -15)                      # APGPU_FAST32_RHO
GUARD_RELEASE = 16                         # APGPU_FAST32_MEAN_GUARD: rms(d) <= |c| / 4
GUARD_OLD = 4                              # the guard before round 6's fix: rms(d) <= |c| / 2
FAST_TAIL = 4                              # kFastTail (full columns)


def fast_tail_padded(np_slots):
    return 6 if np_slots <= 64 else 8


FORMS = ('calib', 'plain')


def slots(n, form='calib'):
    """Slot count, tail length and pads of the fast path for an n-frame stack in the given form: (NP, T, plo, phi)."""
    NP = (n + 3) // 4 * 4
    plo = (NP - n) // 2
    if form == 'plain':
        T = 8 if NP >= 20 else 6
    else:
        T = FAST_TAIL if NP == n else fast_tail_padded(NP)
    return NP, T, plo, NP - n - plo


def fma32(a, b, c):
    """float32 fma(a, b, c) with one rounding: a * b is exact in float64, TwoSum makes p + c = s + e exactly, and s is
    rounded to float32 - except where s sits exactly halfway between two float32 values and e decides the side."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b
        s = p + c
        bp = s - c
        e = (p - bp) + (c - (s - bp))
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        lo = np.nextafter(r, np.float32(-np.inf))
        hi = np.nextafter(r, np.float32(np.inf))
        r = np.where((s == (r64 + hi.astype(np.float64)) / 2) & (e > 0), hi, r)
        r = np.where((s == (r64 + lo.astype(np.float64)) / 2) & (e < 0), lo, r)
    return r.astype(np.float32)


def _pick(V, idx):
    return np.take_along_axis(V, np.asarray(idx)[:, None], axis=1)[:, 0]


def clip_fast32(cols, sigma_lower=3.0, sigma_upper=3.0, maxiters=5, guard=GUARD_RELEASE, form='calib'):
    """The float32 fast clip of `cols` (float32 [M, n]: values in any order, finite) as the fast path of `form` (see the module
    docstring) runs it for an n-frame stack: returns dict(done, a, b, cf, S, Q, NP, T) with the slot indices a, b of the
    sorted, padded column.  done: the lane completes on the fast path (every other lane goes to the exact path)."""
    cols = np.asarray(cols, np.float32)
    M, N = cols.shape
    NP, T, plo, phi = slots(N, form)
    V = np.empty((M, NP), np.float32)
    V[:, :plo] = -np.inf
    V[:, plo:plo + N] = np.sort(cols, axis=1)
    V[:, plo + N:] = np.inf
    with np.errstate(invalid='ignore', over='ignore'):
        cf = V[:, (NP - 1) >> 1].copy()
        Sa = [np.zeros(M, F32) for _ in range(4)]
        Qa = [np.zeros(M, F32) for _ in range(4)]
        for i in range(T, NP // 2):
            d1 = V[:, i] - cf
            d2 = V[:, NP - 1 - i] - cf
            Sa[i & 3] = Sa[i & 3] + (d1 + d2)
            Qa[i & 3] = fma32(d1, d1, Qa[i & 3])
            Qa[(i + 2) & 3] = fma32(d2, d2, Qa[(i + 2) & 3])
        Sc = (Sa[0] + Sa[1]) + (Sa[2] + Sa[3])
        Qc = (Qa[0] + Qa[1]) + (Qa[2] + Qa[3])
        SL = np.zeros((M, T + 1), F32)
        QL = np.zeros((M, T + 1), F32)
        SH = np.zeros((M, T + 1), F32)
        QH = np.zeros((M, T + 1), F32)
        for k in range(T - 1, -1, -1):
            d = V[:, k] - cf
            SL[:, k] = SL[:, k + 1] + d
            QL[:, k] = fma32(d, d, QL[:, k + 1])
        for k in range(1, T + 1):
            d = V[:, NP - T + k - 1] - cf
            SH[:, k] = SH[:, k - 1] + d
            QH[:, k] = fma32(d, d, QH[:, k - 1])
        a = np.full(M, plo)
        b = np.full(M, NP - phi)
        Slo, Qlo = SL[:, plo].copy(), QL[:, plo].copy()
        Shi, Qhi = SH[:, T - phi].copy(), QH[:, T - phi].copy()
        m1 = _pick(V, (a + b - 1) >> 1)
        m2 = _pick(V, (a + b) >> 1)
        vlo, vhi = V[:, plo], V[:, NP - 1 - phi]
        dmax = np.maximum(cf - vlo, vhi - cf)
        unsure = ~((dmax == 0) | ((dmax > F32(2.0 ** -40)) & (dmax < F32(2.0 ** 40))))
        sl4 = F32(4) * F32(float(sigma_lower) ** 2)
        su4 = F32(4) * F32(float(sigma_upper) ** 2)
        rows = np.arange(M)
        it = 0
        while True:
            a0, b0 = a.copy(), b.copy()
            nf = (b - a).astype(F32)
            S = (Sc + Slo) + Shi
            Q = (Qc + Qlo) + Qhi
            nQ = nf * Q
            Vr = fma32(-S, S, nQ)
            unsure |= ~(Vr >= F32(0.25) * nQ)
            tl = sl4 * Vr
            tl_hi, tl_lo = fma32(tl, RHO, tl), fma32(tl, -RHO, tl)

            def t_of(x):
                w = nf * ((x - m1) + (x - m2))
                return w * w
            for I in range(plo, T + 1):
                t = t_of(V[:, I])
                at = a == I
                if I < T:
                    rej = at & (t > tl_hi)
                    unsure |= (at & (t > tl_lo)) != rej
                    a = np.where(rej, I + 1, a)
                    Slo = np.where(rej, SL[:, min(I + 1, T)], Slo)
                    Qlo = np.where(rej, QL[:, min(I + 1, T)], Qlo)
                else:
                    unsure |= at & (t > tl_lo)
            th = su4 * Vr
            th_hi, th_lo = fma32(th, RHO, th), fma32(th, -RHO, th)
            for K in range(T - phi, -1, -1):
                I = NP - T + K - 1
                t = t_of(V[:, I])
                at = b == I + 1
                if K > 0:
                    rej = at & (t > th_hi)
                    unsure |= (at & (t > th_lo)) != rej
                    b = np.where(rej, I, b)
                    Shi = np.where(rej, SH[:, K - 1], Shi)
                    Qhi = np.where(rej, QH[:, K - 1], Qhi)
                else:
                    unsure |= at & (t > th_lo)
            it += 1
            changed = (a != a0) | (b != b0)
            if not (changed.any() and (maxiters is None or maxiters < 0 or it < maxiters)):
                break
            m1 = _pick(V, (a + b - 1) >> 1)
            m2 = _pick(V, (a + b) >> 1)
        low = a > plo
        t = t_of(V[rows, np.maximum(a - 1, 0)])
        unsure |= low & ~(t > tl_hi)
        high = b < NP - phi
        t = t_of(V[rows, np.minimum(b, NP - 1)])
        unsure |= high & ~(t > th_hi)
        S = (Sc + Slo) + Shi
        Q = (Qc + Qlo) + Qhi
        unsure |= ~(F32(guard) * Q <= (b - a).astype(F32) * (cf * cf))
    return dict(done=~unsure, a=a, b=b, cf=cf, S=S, Q=Q, NP=NP, T=T, V=V)


def mean_terms(cf, S, cnt):
    """(cf, ms32): the two float32 terms whose rounded sum is the fast path's mean."""
    nf = np.asarray(cnt).astype(F32)
    y = (F32(1) / nf).astype(F32)                        # v_rcp_f32: exact for powers of two (see the module docstring)
    q0 = (S * y).astype(F32)
    ms32 = fma32(fma32(-nf, q0, S), y, q0)
    return np.asarray(cf, F32), ms32


def exact_model(n):
    """Whether the model is bit-exact for n survivors (the reciprocal of a power of two is exact)."""
    return n > 0 and (n & (n - 1)) == 0


def ulp32(m):
    """ulp of float32 at the magnitude of m (float64): 2^(e - 24) for |m| in [2^(e-1), 2^e)."""
    _, e = np.frexp(np.abs(np.asarray(m, np.float64)))
    return np.ldexp(1.0, e - 24)


def survivors_mean(V, a, b):
    """float64 mean of the sorted survivors V[a .. b) per row (the oracle's mean before its final rounding)."""
    idx = np.arange(V.shape[1])[None, :]
    keep = (idx >= a[:, None]) & (idx < b[:, None])
    x = np.where(keep, V.astype(np.float64), 0.0)
    return x.sum(axis=1) / (b - a)


def evaluate(cols, guard=GUARD_RELEASE, sigma=3.0, maxiters=5, mean_check=True, form='calib'):
    """Everything the search and the tests need per column: done, count, the model's float32 mean, the float64 mean of the
    same survivors, the PRE-ROUNDING error (cf + ms32 - mean) in ulps of the mean, and the rounded result's ulp distance
    from the correctly rounded mean.  mean_check: the kernels' a-posteriori test above 96 slots (False: the guard alone)."""
    r = clip_fast32(cols, sigma_lower=sigma, sigma_upper=sigma, maxiters=maxiters, guard=guard, form=form)
    cnt = r['b'] - r['a']
    cf, ms32 = mean_terms(r['cf'], r['S'], cnt)
    done = r['done']
    with np.errstate(invalid='ignore', over='ignore'):
        pre = cf.astype(np.float64) + ms32.astype(np.float64)       # exact: both terms are float32 of nearby exponents
        if mean_check and r['NP'] > 96:
            # finish_fast_column (stack_kernels.h) above 96 slots: rms(d) > |c| / 8 finishes only within a quarter ulp
            mean = (cf + ms32).astype(F32)
            res = ms32 - (mean - cf)
            wide = ~(F32(64) * r['Q'] <= cnt.astype(F32) * (cf * cf))
            done = done & ~(wide & ~(np.abs(res) <= np.abs(mean) * F32(2.0 ** -26)))
        m = survivors_mean(r['V'], r['a'], r['b'])
        err = (pre - m) / ulp32(m)
        got = (cf + ms32).astype(F32)
        want = m.astype(F32)
        dist = np.abs(_ordered(got) - _ordered(want))
    return dict(done=done, count=cnt, mean=got, mean64=m, err_ulp=err, ulp_dist=dist, cf=cf, ms32=ms32)


def _ordered(x):
    b = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)
