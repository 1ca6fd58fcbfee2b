#!/usr/bin/env python3
"""F9 timing on three 4096 x 4096 planes (a synthetic sky with stars): the quantile levels alone, the composite at V = 1 and V = 9
at 8 and 16 bits, and ApComposite.composite_files end to end (three FITS files in, nine TIFFs out).  Device time by HIP events
(median of --reps); algorithmic GB/s = (12 + 3 V bits / 8) bytes per pixel for the composite and 12 bytes per pixel per read
of the planes (four reads) for the levels, beside a device-to-device copy of the same planes (the copy row of
tools/bench_kernels.py: bytes read + bytes written).

    python tools/bench_composite.py [--size 4096] [--reps 20] [--dir DIR]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = [(gf, cs) for gf in (1.0, 1.2, 1.4) for cs in (1.0, 1.5, 2.0)]


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


def make_planes(size, seed=3):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    planes = 100.0 + 3.0 * torch.randn((3, size, size), generator=g, device='cuda')
    n = size * size // 2000                                                # stars: single bright pixels spread by a 5 x 5 box
    idx = torch.randint(0, size * size, (n,), generator=g, device='cuda')
    amp = 10.0 ** (1.5 + 2.0 * torch.rand((3, n), generator=g, device='cuda'))
    stars = torch.zeros((3, size * size), device='cuda')
    stars.scatter_(1, idx[None].expand(3, -1), amp)
    planes += torch.nn.functional.avg_pool2d(stars.reshape(3, 1, size, size), 5, stride=1, padding=2).reshape(3, size, size) * 25.0
    return planes.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--dir', default=None, help='directory for the end-to-end files (default: a temporary one)')
    p = ap.parse_args()
    import torch
    import astrophotography_amd as apa
    from astrophotography_amd import fitsio, ops
    S = p.size
    npix = S * S
    planes = make_planes(S)
    print('F9 composite: three %d x %d planes; device %s' % (S, S, torch.cuda.get_device_name(0)))
    dst = torch.empty_like(planes)
    med, mn = device_ms(lambda: dst.copy_(planes), p.reps)
    print('  device copy            %8.3f ms median %8.3f ms min  %7.0f GB/s (read + write)' % (med, mn, 2 * 12 * npix / med / 1e6))
    q = [[0.60, 0.999]] * 3
    med, mn = device_ms(lambda: ops.quantile_levels(planes, q), p.reps)
    print('  quantile_levels        %8.3f ms median %8.3f ms min  %7.0f GB/s (four reads of the planes)' % (med, mn, 4 * 12 * npix / med / 1e6))
    levels, n_finite = ops.quantile_levels(planes, q)
    print('    levels %s  finite %s' % (levels.cpu().numpy().round(3).tolist(), n_finite.cpu().tolist()))
    for bits in (8, 16):
        for grid in (GRID[:1], GRID):
            V = len(grid)
            tables = torch.from_numpy(np.stack([ops.tone_table(2.2, gf) for gf, _ in grid])).cuda()
            sat = [cs for _, cs in grid]
            out = torch.empty((V, S, S, 3), dtype=torch.uint8 if bits == 8 else torch.uint16, device='cuda')
            med, mn = device_ms(lambda: ops.composite_rgb(planes, levels, tables, sat, bits=bits, out=out), p.reps)
            nbytes = (12 + 3 * V * bits // 8) * npix
            print('  composite V = %d %2d bit %8.3f ms median %8.3f ms min  %7.0f GB/s (%d bytes per pixel)'
                  % (V, bits, med, mn, nbytes / med / 1e6, nbytes // npix))
            del out
    with tempfile.TemporaryDirectory(dir=p.dir) as d:
        files = []
        for c, name in enumerate(('Red', 'Green', 'Blue')):
            files.append(os.path.join(d, 'bench_%s.fits' % name))
            fitsio.write_device(files[-1], planes[c])
        outs = [os.path.join(d, 'bench_%d.tiff' % v) for v in range(len(GRID))]
        comp = apa.ApComposite('CRITICAL')
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            comp.composite_files(files[0], files[1], files[2], outs, gamma_fac=[1.0, 1.2, 1.4], colour_sat=[1.0, 1.5, 2.0])
            wall.append(time.perf_counter() - t0)
        print('  composite_files        %8.1f ms wall (median of 3; first %.1f): 3 FITS of %.0f MB in, 9 TIFF of %.0f MB out'
              % (1e3 * float(np.median(wall)), 1e3 * wall[0], 4 * npix / 1e6, 3 * npix / 1e6))


if __name__ == '__main__':
    main()
