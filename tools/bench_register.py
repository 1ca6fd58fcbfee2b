#!/usr/bin/env python3
"""F8 timing: 64 frames of 3000 stars on 4096 x 4096 - a dithered sequence with one meridian flip - registered on the first
frame, at K = 40 and K = 64.  Device time of each kernel (HIP events, median of --reps), ops.register_lists end to end (wall
clock with a synchronise) and the NumPy model (tests/register_model.py) on the first --model-frames frames of the same input.

    python tools/bench_register.py [--frames 64] [--stars 3000] [--reps 20] [--model-frames 8]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_sequence(F, n, size=4096, seed=8):
    import register_model as rm
    rng = np.random.default_rng(seed)
    sky = rng.uniform(-200.0, size + 200.0, size=(3 * n, 2))
    rank = rng.permutation(len(sky)).astype(np.float64)
    lists, truth = [], []
    for f in range(F):
        flip = 180.0 if f >= F // 2 else 0.0
        A = rm.make_affine(flip + rng.normal(0.0, 0.2), 1.0 + rng.normal(0.0, 2e-4), shift=rng.uniform(-60.0, 60.0, size=2),
                           centre=((size - 1) / 2.0,) * 2) if f else rm.IDENTITY
        pos = rm.apply_affine(A, sky)
        ok = (pos[:, 0] >= 0) & (pos[:, 0] <= size - 1) & (pos[:, 1] >= 0) & (pos[:, 1] <= size - 1) & (rng.uniform(size=len(sky)) < 0.7)
        ids = np.nonzero(ok)[0]
        ids = ids[np.argsort(rank[ids] + rng.uniform(-6.0, 6.0, size=len(ids)), kind='stable')][:n]
        lists.append(pos[ids] + rng.normal(0.0, 0.1, size=(len(ids), 2)))
        truth.append(A)
    return lists, truth


def device_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--stars', type=int, default=3000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--model-frames', type=int, default=8)
    p = ap.parse_args()
    import torch
    import register_model as rm
    from astrophotography_amd import ops
    lists, truth = make_sequence(p.frames, p.stars)
    xy_h, count_h = rm.pad_lists(lists)
    xy, count = torch.from_numpy(xy_h).cuda(), torch.from_numpy(count_h).cuda()
    print('F8 registration: %d frames x %d stars on 4096^2, one meridian flip; device %s' % (p.frames, p.stars, torch.cuda.get_device_name(0)))
    for K in (40, 64):
        tri = ops.triangle_build(xy, count, K=K)
        ntri = tri['count'].cpu().numpy()
        r = ops.register_lists(xy, count, K=K)
        T = np.where(r['ok'][:, None], r['coeffs'], np.asarray(ops.REGISTER_IDENTITY))
        med_b, min_b = device_ms(lambda: ops.triangle_build(xy, count, K=K), p.reps)
        med_v, min_v = device_ms(lambda: ops.triangle_vote(tri), p.reps)
        med_n, min_n = device_ms(lambda: ops.nearest_match(xy, count, T, 3.0), p.reps)
        wall = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ops.register_lists(xy, count, K=K)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        err = max(rm.corner_error(r['coeffs'][f], truth[f], size=4096) for f in range(p.frames) if r['ok'][f])
        pairs = float(ntri[0]) * float(ntri[1:].sum())
        print('K = %d: triangles per frame %d .. %d (reference %d), %.3g triangle pairs' % (K, ntri.min(), ntri.max(), ntri[0], pairs))
        print('  triangle_build   %8.3f ms median  %8.3f ms min' % (med_b, min_b))
        print('  triangle_vote    %8.3f ms median  %8.3f ms min   %.3g pairs / s' % (med_v, min_v, pairs / (med_v * 1e-3)))
        print('  nearest_match    %8.3f ms median  %8.3f ms min   (radius 3, both directions)' % (med_n, min_n))
        print('  register_lists   %8.3f ms median wall of 5, end to end; %d of %d frames registered, seeds %d .. %d, matched %d .. %d, '
              'largest corner error %.4f px' % (1e3 * float(np.median(wall)), int(r['ok'].sum()), p.frames, r['n_seed'][1:].min(),
                                                r['n_seed'][1:].max(), r['n_matched'][1:].min(), r['n_matched'][1:].max(), err))
        m = min(p.model_frames, p.frames)
        t0 = time.perf_counter()
        want, _ = rm.register_lists(xy_h[:m], count_h[:m], K=K)
        dt = time.perf_counter() - t0
        same = all(np.array_equal(want['pairs'][f], r['pairs'][f]) for f in range(m))
        print('  NumPy model      %8.1f ms for %d of the frames on this host (%.1f ms per frame); same pairs as the device: %s'
              % (1e3 * dt, m, 1e3 * dt / max(1, m - 1), same))


if __name__ == '__main__':
    main()
