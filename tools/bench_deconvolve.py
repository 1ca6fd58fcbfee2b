#!/usr/bin/env python3
"""F12 timing on one 4096 x 4096 image: the forward + ratio kernel and the back-projection + update kernel per iteration, and 30
iterations of ops.richardson_lucy end to end, at radius 2, 6 and 12, undamped (T = 0) and damped (T = 3).  Device time by HIP events
(one warm-up call, then the median, minimum and maximum of --reps calls).

Each kernel is set against two floors:
  HBM   the algorithmic bytes, 12 B per pixel forward (u and d read, r written) and 16 B per pixel backward (r, u, inv read, u'
        written), at the rate of a device-to-device copy measured in the same run;
  VALU  2 K^2 vector operations per pixel and pass (a multiply and an add per tap, no FMA: they round separately), on 256 CUs x 4
        SIMDs x 16 lanes at the shader clock read in the same run.  Packed two-wide float32 operations would halve it; the floor is
        stated for one operation per lane and cycle.

    python tools/bench_deconvolve.py [--size 4096] [--reps 10]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES = 256 * 4 * 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=10)
    p = ap.parse_args()
    import torch
    from astrophotography_amd import ops
    size = p.size
    npix = size * size
    khz = getattr(torch.cuda.get_device_properties(0), 'clock_rate', 0)       # the device's peak shader clock, kHz
    clock_mhz = khz / 1e3 if khz else 2400.0
    print('F12 Richardson-Lucy; device %s; shader clock %d MHz (%s); %d repetitions after one warm-up call' % (
        torch.cuda.get_device_name(0), clock_mhz, 'device properties' if khz else 'nominal: the properties give none', p.reps))
    g = torch.Generator(device='cuda').manual_seed(5)
    d = (300.0 + 17.0 * torch.randn((size, size), generator=g, device='cuda')).contiguous()
    d[torch.rand((size, size), generator=g, device='cuda') < 0.01] = float('nan')
    u = (200.0 + 5.0 * torch.randn((size, size), generator=g, device='cuda')).abs().contiguous()
    r, u2, out = torch.empty_like(d), torch.empty_like(d), torch.empty_like(d)
    ws = ops.deconv_workspace(d.shape, 'cuda')
    print('1 image of %d x %d' % (size, size))
    copy = device_ms(lambda: out.copy_(d), p.reps)
    copy_gbs = 8 * npix / copy[0] / 1e6
    print('  device copy of 4 bytes per pixel (read + write)      %8.3f ms median (%7.3f .. %7.3f)  %6.0f GB/s' % (copy + (copy_gbs,)))
    for R in (2, 6, 12):
        K = 2 * R + 1
        psf = ops.psf_gaussian(R / 1.7, R)
        inv = ops.deconv_norm(d, psf)
        valu_ms = 2.0 * K * K * npix / (LANES * clock_mhz * 1e6) * 1e3
        print('radius %d (%d x %d taps): VALU floor %.3f ms per pass; norm %.3f ms' % (
            R, K, K, valu_ms, device_ms(lambda: ops.deconv_norm(d, psf, out=out), p.reps)[0]))
        for T in (0.0, 3.0):
            fwd = device_ms(lambda: ops.deconv_ratio(u, d, psf, 100.0, 1.5, 4.0, T, out=r), p.reps)
            bwd = device_ms(lambda: ops.deconv_update(u, r, inv, psf, out=u2), p.reps)
            for label, ms, nbytes in (('forward + ratio', fwd, 12 * npix), ('back-projection + update', bwd, 16 * npix)):
                hbm_ms = nbytes / copy_gbs / 1e6
                floor = max(hbm_ms, valu_ms)
                print('  T = %g %-26s %8.3f ms median (%7.3f .. %7.3f)  HBM floor %6.3f ms, VALU floor %6.3f ms: %s binds, %4.1f x the floor' % (
                    T, label, ms[0], ms[1], ms[2], hbm_ms, valu_ms, 'VALU' if valu_ms > hbm_ms else 'HBM', ms[0] / floor))
            full = device_ms(lambda: ops.richardson_lucy(d, psf, 100.0, 30, T, 1.5, 4.0, start=200.0, ws=ws, out=out), max(3, p.reps // 3))
            print('  T = %g 30 iterations end to end     %8.3f ms median (%7.3f .. %7.3f)  %.3f ms per iteration' % (
                T, full[0], full[1], full[2], full[0] / 30.0))


if __name__ == '__main__':
    main()
