// stack_reject_walk.inc - a FRAGMENT of the rejection kernels (stack_reject.hip, stack_esd.hip), included inside the kernel body
// behind the final statistics: the weighted mean of APGPU_STACK_FRAME_PARAMS / APGPU_STACK_FRAME_LOCAL.  Text, not a function
// (see stack_reject_load.inc).  In scope: RawT, LOC, WT; prm, N, base, lane, valid, cell, cells; the membership test of the rule
// - mm_klo, mm_khi, mm_dlo, mm_keephi, mm_some (min/max: prm.minmax != 0) or Lo, Hi (Winsorized) -; mean, which it sets.
    // ---- (FP) the weighted mean.  The compact column has lost its frame indices, so the frames are walked once more from memory
    // (the kernel is bound by its arithmetic many times over, DESIGN 4.1e): v is formed again, the rule's membership test is
    // repeated on it - Winsorized: finite and inside [Lo, Hi], for a removed value lies outside its round's interval and a kept one
    // inside every round's; min/max: the two key bounds and the tie counters over the finite values in frame order, as the
    // compaction above counted them - and num += double(w) double(v), den += double(w) run in frame order from +0.
    if constexpr (WT) {
        const int off = valid ? lane : 0;
        const RawT *const fb = static_cast<const RawT *>(prm.frames) + base + off;
        const bool mm = prm.minmax != 0;
        double num = 0.0, den = 0.0;
        int seenlo = 0, seenhi = 0;
        constexpr int B = 8;                                 // frames per block: eight loads in flight, as on the first load
#pragma unroll 1
        for (int j = 0; j < N; j += B) {
            RawT raw[B];
#pragma unroll
            for (int k = 0; k < B; k++) {
                const int f = j + k < N ? j + k : N - 1;
                raw[k] = fb[(int64_t)f * prm.stride];
            }
#pragma unroll
            for (int k = 0; k < B; k++) {
                const int f = j + k < N ? j + k : N - 1;
                float x, w;
                if constexpr (LOC) {
                    x = local_map(to_f32(raw[k]), prm.lscale, prm.loffset, cells, f, cell);
                    w = prm.lweight ? prm.lweight[f] : 1.f;
                } else {
                    x = frame_map(to_f32(raw[k]), prm.exp_ratio[f], prm.exp_ratio[N + f]);
                    w = prm.exp_ratio[2 * N + f];
                }
                const bool fin = j + k < N && is_finite(x);
                bool ok;
                if (mm) {                                    // (wave-uniform)
                    const unsigned key = OrderKey<float>::to(x);
                    const bool elo = key == mm_klo, ehi = key == mm_khi;
                    ok = fin && mm_some && key >= mm_klo && (!elo || seenlo >= mm_dlo) && key <= mm_khi && (!ehi || seenhi < mm_keephi);
                    seenlo += (elo && fin) ? 1 : 0;
                    seenhi += (ehi && fin) ? 1 : 0;
                } else {
                    const double xd = widen(x);
                    ok = fin && xd >= Lo && xd <= Hi;
                }
                const double wd = widen(w);
                const double t = wd * widen(x);              // (exact: two widened float32 values)
                num = ok ? num + t : num;
                den = ok ? den + wd : den;
            }
        }
        mean = num / den;
    }
