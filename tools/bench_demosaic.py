#!/usr/bin/env python3
"""F10 timing: the four demosaic methods x uint16 / float32 mosaics x RGB_F32 / RGB_U16 / GREY_F32 on one 4096 x 4096 frame and on
a 16-frame slab of 2048 x 2048, and bayer_channel_sums.  Device time by HIP events (one warm-up call, then the median, minimum and
maximum of --reps calls); algorithmic GB/s = (bytes of the mosaic read once + bytes written) / time, beside the 8 TB/s HBM peak and
a device-to-device copy of 12 bytes per pixel.

    python tools/bench_demosaic.py [--size 4096] [--shape 4176 6248] [--slab 16 2048] [--reps 20] [--methods mhc rcd]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0
METHODS = ('bilinear', 'mhc', 'superpixel', 'rcd')
OUTPUTS = (('rgb', 12), ('rgb_u16', 6), ('grey', 4))        # bytes written per output pixel


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


def make_mosaic(n, shape, dtype, seed=5):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    m = (1200.0 + 300.0 * torch.randn((n,) + tuple(shape), generator=g, device='cuda')).clamp_(0, 65535)
    if dtype == 'u16':
        return m.to(torch.int32).to(torch.int16).view(torch.uint16).contiguous()
    return m.contiguous()


def row(label, ms, nbytes):
    med, mn, mx = ms
    gbs = nbytes / med / 1e6
    print('  %-44s %8.3f ms median (%7.3f .. %7.3f)  %7.0f GB/s  %4.1f %% of peak' % (label, med, mn, mx, gbs, 100.0 * gbs / PEAK_GBS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--shape', type=int, nargs=2, default=None, metavar=('ROWS', 'COLUMNS'), help='one frame of this shape instead of --size squared')
    ap.add_argument('--methods', nargs='+', default=list(METHODS), choices=METHODS)
    ap.add_argument('--slab', type=int, nargs=2, default=[16, 2048], metavar=('FRAMES', 'SIZE'))
    ap.add_argument('--reps', type=int, default=20)
    p = ap.parse_args()
    import torch
    from astrophotography_amd import ops
    print('F10 demosaic; device %s; %d repetitions after one warm-up call' % (torch.cuda.get_device_name(0), p.reps))
    pattern, black, gain = (0, 1, 3, 2), [256, 256, 256, 256], [1.9, 1.0, 1.5, 1.0]
    for n, shape in ((1, tuple(p.shape) if p.shape else (p.size, p.size)), (p.slab[0], (p.slab[1], p.slab[1]))):
        npix = n * shape[0] * shape[1]
        print('%d frame(s) of %d x %d' % (n, shape[0], shape[1]))
        src = torch.empty((3, npix), dtype=torch.float32, device='cuda')
        dst = torch.empty_like(src)
        row('device copy of 12 bytes per pixel (read + write)', device_ms(lambda: dst.copy_(src), p.reps), 24 * npix)
        del src, dst
        for dtype, in_bytes in (('u16', 2), ('f32', 4)):
            m = make_mosaic(n, shape, dtype)
            for method in p.methods:
                if method == 'superpixel' and (shape[0] % 2 or shape[1] % 2):
                    continue
                scale = 4 if method == 'superpixel' else 1
                for output, out_bytes in OUTPUTS:
                    out = ops.bayer_demosaic(m, pattern, black, gain, method, output)
                    ms = device_ms(lambda: ops.bayer_demosaic(m, pattern, black, gain, method, output, out=out), p.reps)
                    row('%-10s %s -> %-7s (%4.1f B per pixel)' % (method, dtype, output, in_bytes + out_bytes / scale), ms,
                        npix * in_bytes + npix * out_bytes // scale)
                    del out
            out = ops.bayer_demosaic(m, pattern, black, gain, 'mhc', 'direct')
            row('direct     %s -> f32     (%4.1f B per pixel)' % (dtype, in_bytes + 4),
                device_ms(lambda: ops.bayer_demosaic(m, pattern, black, gain, 'mhc', 'direct', out=out), p.reps), npix * (in_bytes + 4))
            del out
            if n == 1:
                row('channel_sums %s, whole image' % dtype, device_ms(lambda: ops.bayer_channel_sums(m[0], pattern, black), p.reps), npix * in_bytes)
            del m


if __name__ == '__main__':
    main()
