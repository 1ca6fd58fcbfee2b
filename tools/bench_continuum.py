#!/usr/bin/env python3
"""F11 timing on one 4096 x 4096 image: the normalised Gaussian blur at radius 2, 8 and 32, one launch of the six moments, the fused
subtraction, and ApContinuumSubtract.subtract end to end (PSF matching + clipped pixel fit + subtraction; wall time, it reads the
moments back every round).  Device time by HIP events (one warm-up call, then the median, minimum and maximum of --reps calls);
algorithmic GB/s = bytes / time: the blur 8 B per pixel (one read, one write), the moments 8 B per pixel (two reads), the subtraction
12 B per pixel; beside the 8 TB/s HBM peak and a device-to-device copy of 4 bytes per pixel.

    python tools/bench_continuum.py [--size 4096] [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0


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
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def row(label, ms, nbytes):
    med, mn, mx = ms
    gbs = nbytes / med / 1e6
    print('  %-52s %8.3f ms median (%7.3f .. %7.3f)  %7.0f GB/s  %4.1f %% of peak' % (label, med, mn, mx, gbs, 100.0 * gbs / PEAK_GBS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    p = ap.parse_args()
    import torch
    import astrophotography_amd as apg
    from astrophotography_amd import ops
    print('F11 continuum subtraction; device %s; %d repetitions after one warm-up call' % (torch.cuda.get_device_name(0), p.reps))
    size = p.size
    npix = size * size
    g = torch.Generator(device='cuda').manual_seed(5)
    c = (30.0 + 1.5 * torch.randn((size, size), generator=g, device='cuda')).contiguous()
    n = (0.083 * c + 0.4 + 0.5 * torch.randn((size, size), generator=g, device='cuda')).contiguous()
    n[torch.rand((size, size), generator=g, device='cuda') < 0.01] = float('nan')
    out = torch.empty_like(c)
    print('1 image of %d x %d' % (size, size))
    row('device copy of 4 bytes per pixel (read + write)', device_ms(lambda: out.copy_(c), p.reps), 8 * npix)
    for R in (2, 8, 32):
        taps = ops.gauss_taps(R / 4.0, R)
        row('gauss_blur radius %2d (%2d taps, 8 B per pixel)' % (R, 2 * R + 1), device_ms(lambda: ops.gauss_blur(n, taps, 0.5, out=out), p.reps),
            8 * npix)
    ws = torch.empty(_ws_bytes(npix), dtype=torch.uint8, device='cuda')
    row('pair_moments, one launch (8 B per pixel)', device_ms(lambda: ops.pair_moments(n, c, 0.083, 0.4, -1.8, 1.2, ws=ws), p.reps), 8 * npix)
    row('linear_combine (12 B per pixel)', device_ms(lambda: ops.linear_combine(n, c, 1.0, -0.083, -0.4, out=out), p.reps), 12 * npix)
    cs = apg.ApContinuumSubtract('ERROR', method='pixels')
    cs.subtract(n, c, fwhm=(2.6, 3.4))
    torch.cuda.synchronize()
    walls = []
    for _ in range(max(3, p.reps // 4)):
        t0 = time.perf_counter()
        r = cs.subtract(n, c, fwhm=(2.6, 3.4))
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    print('  %-52s %8.3f ms median wall (%7.3f .. %7.3f); %d clipping rounds, radius-%d blur' % (
        'ApContinuumSubtract.subtract, FWHM 2.6 and 3.4', float(np.median(walls)), min(walls), max(walls), r['report']['iterations'],
        (r['report']['taps'] - 1) // 2))


def _ws_bytes(npix):
    from astrophotography_amd import _lib
    return _lib.load().apgpu_pair_moments_ws_bytes(npix)


if __name__ == '__main__':
    main()
