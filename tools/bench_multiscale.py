#!/usr/bin/env python3
"""F13 timing on one 4096 x 4096 image: one launch of the starlet step at every spacing s = 1 .. 32, in each form the spacing has
(tile: LDS, s <= 8; direct: register chains, any s; '*' marks the one the library picks), and ops.multiscale end to end for J = 4
and J = 6.  Device time by HIP events around a batch of calls (one warm-up batch, then the median, minimum and maximum of --reps
batches, per call).

Each time is set against the algorithmic bytes - 12 B per pixel for a first step (c_j read, c_{j+1} and the
accumulator written), 16 B for a later one (the accumulator read as well), 12 B for the last step of a whole call (c_J is not
stored), 8 B when the only step is both - at the 8 TB/s of the data sheet and at the rate of a device-to-device copy measured in
the same run.

    python tools/bench_multiscale.py [--size 4096] [--reps 10] [--batch 20]
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
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=20)
    p = ap.parse_args()
    import torch
    from astrophotography_amd import _lib, ops
    size = p.size
    npix = size * size
    print('F13 starlet; device %s; %d batches of %d calls after one warm-up batch' % (torch.cuda.get_device_name(0), p.reps, p.batch))
    g = torch.Generator(device='cuda').manual_seed(5)
    d = (300.0 + 17.0 * torch.randn((size, size), generator=g, device='cuda')).contiguous()
    d[torch.rand((size, size), generator=g, device='cuda') < 0.01] = float('nan')
    c, acc, out = torch.empty_like(d), torch.zeros_like(d), torch.empty_like(d)
    ws = ops.starlet_workspace(d.shape, 'cuda')
    print('1 image of %d x %d, 1 %% holes' % (size, size))
    copy = device_ms(lambda: out.copy_(d), p.reps, p.batch)
    copy_gbs = 8 * npix / copy[0] / 1e6
    print('  device copy of 4 bytes per pixel (read + write)   %8.4f ms median (%7.4f .. %7.4f)  %6.0f GB/s' % (copy + (copy_gbs,)))

    def line(label, ms, nbytes):
        gbs = nbytes / ms[0] / 1e6
        print('  %-48s %8.4f ms median (%7.4f .. %7.4f)  %2d B/pixel  %6.0f GB/s = %4.1f %% of 8 TB/s, %5.1f %% of the copy rate' % (
            label, ms[0], ms[1], ms[2], nbytes // npix, gbs, gbs / 80.0, 100.0 * gbs / copy_gbs))

    for s in (1, 2, 4, 8, 16, 32):
        auto = 'tile' if s <= _lib.STARLET_TILE_MAX_AUTO else 'direct'
        for form in (('tile', 'direct') if s <= _lib.STARLET_TILE_MAX_SPACING else ('direct',)):
            for first in ((True, False) if s == 1 else (False,)):
                ms = device_ms(lambda: ops.starlet_step(d, s, out=c, acc=acc, threshold=40.0, gain=1.0, first=first, form=form), p.reps, p.batch)
                line('step s = %2d %-6s %s%s' % (s, form, 'first step' if first else 'later step', ' *' if form == auto else ''), ms,
                     (12 if first else 16) * npix)
    ms = device_ms(lambda: ops.starlet_plane1(d, out=c), p.reps, p.batch)
    line('plane 1 alone', ms, 8 * npix)
    for J in (4, 6):
        ms = device_ms(lambda: ops.multiscale(d, J, (3.0, 3.0, 2.0, 1.0, 1.0, 1.0)[:J], 1.0, 1.0, 'hard', sigma=17.0, ws=ws, out=out), p.reps,
                       max(1, p.batch // 4))
        line('multiscale J = %d, %d launches, sigma given' % (J, J), ms, (12 + 16 * (J - 2) + 12) * npix)
    ms = device_ms(lambda: ops.multiscale(d, 4, ws=ws, out=out), max(3, p.reps // 3), 1)
    print('  multiscale J = 4 with the noise measured (plane 1 + sigclip_global + host read-back)   %8.3f ms median (%7.3f .. %7.3f)' % ms)


if __name__ == '__main__':
    main()
