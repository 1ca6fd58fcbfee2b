// stack_reject_load.inc - a FRAGMENT of the rejection kernels (stack_reject.hip, stack_esd.hip), included inside the kernel body:
// the lane's place in the meshes and the load of its column.  Text, not a function: the kernels of stack_reject.hip keep, token
// for token, the code their recorded measurements were taken with.  In scope: NP, RawT, CALIB, FP, LOC; prm (RejectParams), N,
// base, lane, valid, cell, cells, v[NP].
    if constexpr (LOC) {                                     // (a lane behind the last pixel takes the block's first one)
        const int64_t q = base + (valid ? lane : 0);
        const int64_t row = q / prm.width;
        const int y = (int)(prm.row0 + row), x = (int)(q - row * prm.width);
        int j0, j1, k0, k1;
        mesh_axis(y, prm.bh, prm.ny, j0, j1, cell.ty);
        mesh_axis(x, prm.bw, prm.nx, k0, k1, cell.tx);
        cell.i00 = j0 * prm.nx + k0; cell.i01 = j0 * prm.nx + k1;
        cell.i10 = j1 * prm.nx + k0; cell.i11 = j1 * prm.nx + k1;
        cells = (int64_t)prm.ny * prm.nx;
    }

    // ---- the column: load, calibrate (stack_calibrate.h, load_column_exact: IEEE division, one value at a time) ----
    {
        const int off = valid ? lane : 0;
        float b = 0.f, D = 0.f, nf = 1.f;
        bool dodiv = false;
        if constexpr (CALIB) {
            b = prm.bias[base + off];
            const float d = prm.dark[base + off];
            D = prm.still_biased ? d - b : d;                // ApCalibrate.py:440-445
            if (prm.nflat) {
                nf = prm.nflat[base + off];
                dodiv = (nf != 0.f);                         // ApCalibrate.py:462 (NaN != 0 is True)
            }
        }
        const RawT *const fb = static_cast<const RawT *>(prm.frames) + base + off;
#pragma unroll
        for (int j = 0; j < NP; j += 8) {                    // blocks of 8 frames: eight loads in flight, one branch
            if (j >= N) {                                    // (wave-uniform)
#pragma unroll
                for (int k = 0; k < 8; k++) v[j + k] = quiet_nan();
                continue;
            }
            RawT raw[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int f = j + k < N ? j + k : N - 1;     // slots behind the last frame re-read it and are then dropped
                raw[k] = fb[(int64_t)f * prm.stride];
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int f = j + k < N ? j + k : N - 1;
                float x = to_f32(raw[k]);
                if constexpr (CALIB) {
                    const float e = prm.exp_ratio[f];
                    const float ped = prm.pedestal ? prm.pedestal[f] : 0.f;
                    if (ped != 0.f) x = x + ped;             // ApCalibrate.py:318-326
                    x = x - b;                               // :439
                    const float ds = e * D;                  // :450
                    x = x - ds;                              // :451
                    if (dodiv) x = __fdiv_rn(x, nf);         // :463
                }
                if constexpr (FP) x = frame_map(x, prm.exp_ratio[f], prm.exp_ratio[N + f]);
                if constexpr (LOC) x = local_map(x, prm.lscale, prm.loffset, cells, f, cell);
                v[j + k] = j + k < N ? x : quiet_nan();
            }
        }
    }
