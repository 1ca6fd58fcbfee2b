#!/usr/bin/env python3
"""F14 timing: N = 16 and 64 frames of 4096 x 4096 drizzled onto 8192 x 8192 (s = 2, p = 0.5) - plain, with masks (a shared mask and
frame masks), as one CFA plane - the rejection kernel, the device part of ApDrizzle.drizzle with rejection and background weights end
to end, and beside them ops.coadd(combine='AVERAGE', out_shape=(8192, 8192)) with the same composed transforms: the only way onto a
finer grid before F14.  Device time by HIP events around a batch of calls (one warm-up batch, then the median, minimum and maximum
of --reps batches, per call).

The drizzle is set against its algorithmic bytes, 4 N H W read + 8 s^2 H W written, at the 8 TB/s of the data sheet and at the rate
of a device-to-device copy measured in the same run; the rejection against 5 N H W (frames read, flags written).

    python tools/bench_drizzle.py [--size 4096] [--frames 16,64] [--reps 5] [--batch 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_ms(fn, reps, batch):
    import torch
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / batch)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--frames', default='16,64')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=3)
    p = ap.parse_args()
    import torch
    import astrophotography_amd as apkg
    from astrophotography_amd import ops
    H = W = p.size
    s, pf = 2.0, 0.5
    h, w = int(H * s), int(W * s)
    print('F14 drizzle; device %s; %d batches of %d calls after one warm-up batch' % (torch.cuda.get_device_name(0), p.reps, p.batch))
    g = torch.Generator(device='cuda').manual_seed(5)
    a = torch.empty((h, w), device='cuda')
    b = torch.empty_like(a)
    copy = device_ms(lambda: b.copy_(a), p.reps, 10)
    copy_gbs = 8.0 * h * w / copy[0] / 1e6
    print('device copy of %d x %d float32 (read + write)  %8.3f ms median (%7.3f .. %7.3f)  %6.0f GB/s' % ((h, w) + copy + (copy_gbs,)))
    del a, b
    rng = np.random.default_rng(7)
    for N in [int(v) for v in p.frames.split(',')]:
        frames = torch.empty((N, H, W), device='cuda')
        for f in range(N):
            frames[f] = torch.randn((H, W), generator=g, device='cuda') * 17.0 + 300.0
        th = np.deg2rad(rng.uniform(-0.2, 0.2, N))
        aff = np.stack([np.cos(th), -np.sin(th), rng.uniform(-3, 3, N), np.sin(th), np.cos(th), rng.uniform(-3, 3, N)], 1)
        mask = (torch.rand((H, W), generator=g, device='cuda') < 0.001).to(torch.uint8)
        fmask = torch.zeros((N, H, W), dtype=torch.uint8, device='cuda')
        for f in range(N):
            fmask[f] = (torch.rand((H, W), generator=g, device='cuda') < 0.001).to(torch.uint8)
        nbytes = 4.0 * N * H * W + 8.0 * h * w
        print('%d frames of %d x %d onto %d x %d, s = 2, p = 0.5; algorithmic bytes %.3f GB' % (N, H, W, h, w, nbytes / 1e9))

        def row(name, fn, nb=nbytes):
            t = device_ms(fn, p.reps, p.batch)
            floor8, floorc = nb / 8e12 * 1e3, nb / (copy_gbs * 1e9) * 1e3
            print('  %-44s %9.3f ms median (%8.3f .. %8.3f)  %5.1f %% of the floor at 8 TB/s, %5.1f %% at the copy rate'
                  % ((name,) + t + (100.0 * floor8 / t[0], 100.0 * floorc / t[0])))
            return t[0]

        row('drizzle', lambda: ops.drizzle(frames, aff, s, pf))
        row('drizzle, shared mask + frame masks', lambda: ops.drizzle(frames, aff, s, pf, mask=mask, frame_masks=fmask), nbytes + N * H * W + H * W)
        row('drizzle, CFA plane G of RGGB', lambda: ops.drizzle(frames, aff, s, pf, cfa=((0, 1, 3, 2), 1)))
        row('drizzle, CFA plane R of RGGB', lambda: ops.drizzle(frames, aff, s, pf, cfa=((0, 1, 3, 2), 0)))
        ref = ops.coadd(frames[:8], aff[:8], combine='MEDIAN')['image']
        sig = np.full(N, 17.0)
        row('drizzle_reject against a scale-1 reference', lambda: ops.drizzle_reject(frames, aff, ref, 1.0, sigmas=sig), 5.0 * N * H * W)
        dz = apkg.ApDrizzle('ERROR', scale=s, pixfrac=pf, reject=True)
        if N <= 16:
            row('ApDrizzle.drizzle: weights, median, flags, drizzle', lambda: dz.drizzle(frames, aff))
        fine = ops.drizzle_affines(aff, s)
        if N <= 16:
            row("ops.coadd(combine='AVERAGE') onto %d x %d" % (h, w), lambda: ops.coadd(frames, fine, out_shape=(h, w), combine='AVERAGE'),
                4.0 * N * H * W + 4.0 * h * w)
        else:
            print("  ops.coadd(combine='AVERAGE') onto %d x %d: not run, its resampled slab would be %.0f GB" % (h, w, 4.0 * N * h * w / 1e9))
        del frames, fmask, mask, ref
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
