#!/usr/bin/env python3
"""F20 timing on one 4096 x 4096 image: the three kernels of csrc/gradient.hip and ApRemoveGradient.remove end to end.

  sample statistics  K = 256 and 4096 boxes of radius 12 and 32, with a mask: algorithmic bytes K (2 r + 1)^2 5 (a float32 and a mask byte
                     per box pixel, read once; the passes after the first walk LDS)
  surface lattice    a thin-plate spline of K = 256, 1024 and 4096 centres on the 260 x 260 nodes of step 16: K terms per node, a
                     float64 log each - no bytes to speak of, so terms per second
  apply              8 B per pixel, 12 B with the surface plane
  composed           the same result from what the library had before: ops.spline_zoom of a 16 x 16 mesh to a float64 plane (8 B per
                     pixel written), then torch arithmetic (image to float64, minus, plus, back to float32)
  end to end         ApRemoveGradient.remove, wall time (source mask, samples, host fit, lattice, apply), poly and tps

Device time by HIP events (one warm-up call, then the median, minimum and maximum of --reps calls); GB/s = algorithmic bytes / time,
beside the 8 TB/s HBM peak and a device-to-device copy of 4 bytes per pixel measured in the same run.

    python tools/bench_gradient.py [--size 4096] [--reps 20]
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


def row(label, ms, nbytes, copy_gbs=None):
    med, mn, mx = ms
    gbs = nbytes / med / 1e6
    tail = '' if copy_gbs is None else '  %5.1f %% of the copy rate' % (100.0 * gbs / copy_gbs)
    print('  %-58s %8.3f ms median (%7.3f .. %7.3f)  %7.0f GB/s  %4.1f %% of peak%s' % (label, med, mn, mx, gbs, 100.0 * gbs / PEAK_GBS, tail))
    return gbs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    p = ap.parse_args()
    import torch
    import astrophotography_amd as apg
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApMeasureBackground import _bspline3_prefilter
    print('F20 sky gradient; device %s; %d repetitions after one warm-up call' % (torch.cuda.get_device_name(0), p.reps))
    size = p.size
    npix = size * size
    g = torch.Generator(device='cuda').manual_seed(20)
    yy, xx = torch.meshgrid(torch.arange(size, device='cuda', dtype=torch.float32), torch.arange(size, device='cuda', dtype=torch.float32), indexing='ij')
    img = (1000.0 + 0.02 * xx - 0.015 * yy + 5.0 * torch.randn((size, size), generator=g, device='cuda')).contiguous()
    img[torch.rand((size, size), generator=g, device='cuda') < 0.001] = float('nan')
    mask = (torch.rand((size, size), generator=g, device='cuda') < 0.05).to(torch.uint8)
    out, surf = torch.empty_like(img), torch.empty_like(img)
    print('1 image of %d x %d' % (size, size))
    copy = row('device copy of 4 bytes per pixel (read + write)', device_ms(lambda: out.copy_(img), p.reps), 8 * npix)
    rng = np.random.default_rng(1)
    for K in (256, 4096):
        per_row = int(round(K ** 0.5))
        c = torch.from_numpy(ops.gradient_samples((size, size), per_row)).cuda()
        assert c.shape[0] == K
        for r in (12, 32):
            row('sample_clipped_stats K %4d radius %2d (%4d px a box)' % (K, r, (2 * r + 1) ** 2),
                device_ms(lambda: ops.sample_clipped_stats(img, mask, c, r), p.reps), K * (2 * r + 1) ** 2 * 5, copy)
    frame = ops.surface_frame((size, size))
    ny = nx = (size - 1) // 16 + 4
    for K in (256, 1024, 4096):
        tps = dict(model='tps', a=np.array([1000.0, 40.0, -30.0]), w=rng.normal(0, 5.0, K), uv=rng.uniform(-1, 1, (K, 2)), frame=frame)
        med, mn, mx = device_ms(lambda: ops.surface_lattice(tps, (size, size), 16), p.reps)
        print('  %-58s %8.3f ms median (%7.3f .. %7.3f)  %7.2f G terms/s (%d x %d nodes)' % ('surface_lattice tps K %4d, step 16 (with the upload)' % K, med, mn, mx,
                                                                                            ny * nx * K / med / 1e6, ny, nx))
    poly = dict(model='poly', degree=3, coef=rng.normal(0, 10.0, 10) + 100.0, frame=frame)
    med, mn, mx = device_ms(lambda: ops.surface_lattice(poly, (size, size), 16), p.reps)
    print('  %-58s %8.3f ms median (%7.3f .. %7.3f)' % ('surface_lattice poly degree 3, step 16 (with the upload)', med, mn, mx))
    lat = ops.surface_lattice(poly, (size, size), 16)
    for step in (16, 64):
        lt = ops.surface_lattice(poly, (size, size), step)
        row('surface_apply subtract, step %2d (8 B per pixel)' % step, device_ms(lambda: ops.surface_apply(img, lt, step, 'subtract', 100.0, out=out), p.reps),
            8 * npix, copy)
    row('surface_apply divide, step 16 (8 B per pixel)', device_ms(lambda: ops.surface_apply(img, lat, 16, 'divide', 100.0, out=out), p.reps), 8 * npix, copy)
    row('surface_apply subtract + surface plane (12 B per pixel)',
        device_ms(lambda: ops.surface_apply(img, lat, 16, 'subtract', 100.0, out=out, surface_out=surf), p.reps), 12 * npix, copy)
    row('surface_apply in place (8 B per pixel)', device_ms(lambda: ops.surface_apply(out, lat, 16, 'subtract', 0.0, out=out), p.reps), 8 * npix, copy)
    # what a user could do before: a float64 plane from the spline zoom of a mesh, then torch arithmetic
    box = size // 16
    mesh = 1000.0 + rng.normal(0, 10.0, (16, 16))
    coef = torch.from_numpy(_bspline3_prefilter(mesh)).cuda()

    def composed():
        bg = ops.spline_zoom(coef, box, box, size, size, float(mesh.min()), float(mesh.max()))
        return (img.double() - bg + 100.0).float()
    row('composed: spline_zoom + torch arithmetic (same 8 B per pixel)', device_ms(composed, p.reps), 8 * npix, copy)
    rg = apg.ApRemoveGradient('ERROR')
    for model in ('poly', 'tps'):
        rg.remove(img, model=model)
        torch.cuda.synchronize()
        walls = []
        for _ in range(max(3, p.reps // 4)):
            t0 = time.perf_counter()
            r = rg.remove(img, model=model)
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        print('  %-58s %8.3f ms median wall (%7.3f .. %7.3f); %d of %d samples kept' % ('ApRemoveGradient.remove %s, source mask included' % model,
                                                                                       float(np.median(walls)), min(walls), max(walls), r['kept'].sum(), len(r['kept'])))
    m = rg.source_mask(img)
    walls = []
    for _ in range(max(3, p.reps // 4)):
        t0 = time.perf_counter()
        rg.remove(img, mask=m)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    print('  %-58s %8.3f ms median wall (%7.3f .. %7.3f)' % ('ApRemoveGradient.remove poly, the mask given', float(np.median(walls)), min(walls), max(walls)))


if __name__ == '__main__':
    main()
