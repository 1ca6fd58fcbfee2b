#!/usr/bin/env python3
"""F19 timing (DESIGN 4.3e'): what carrying a distortion map costs next to one affine per frame.

  drizzle          16 frames of 4096 x 4096 onto 8192 x 8192 (s = 2, p = 0.5): one transform per frame against the same transforms
                   replicated into every 16 x 64 output tile, the two forms interleaved call by call in one run
  resample_affine  16 frames of 4096 x 4096, per frame against per tile (existing kernels; record only)
  tile affines     ops.poly_tile_affines for 64 frames of 4096 x 4096, degree 3 and 5 (the estimate on the host is part of the call)
  register_lists   'affine' against 'poly3' on tools/bench_register.py's lists (wall clock)

Device time by HIP events around single calls, median and range of --reps; the interleaved pairs alternate A B A B.

    python tools/bench_distortion.py [--size 4096] [--frames 16] [--reps 7]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def interleaved_ms(fns, reps):
    """{name: (median, min, max)} of device time per call, the calls of `fns` (name -> callable) alternating."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def show(rows):
    for k, (med, lo, hi) in rows.items():
        print('  %-46s %9.3f ms median (%8.3f .. %8.3f)' % (k, med, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--reps', type=int, default=7)
    p = ap.parse_args()
    import torch
    import register_model as rm
    from astrophotography_amd import ops
    from astrophotography_amd.distortion import PolyMap
    from bench_register import make_sequence
    H = W = p.size
    N, s, pf = p.frames, 2.0, 0.5
    print('F19 lens distortion; device %s; %d repetitions per row' % (torch.cuda.get_device_name(0), p.reps))
    g = torch.Generator(device='cuda').manual_seed(5)
    rng = np.random.default_rng(7)
    frames = torch.empty((N, H, W), device='cuda')
    for f in range(N):
        frames[f] = torch.randn((H, W), generator=g, device='cuda') * 17.0 + 300.0
    th = np.deg2rad(rng.uniform(-0.2, 0.2, N))
    aff = np.stack([np.cos(th), -np.sin(th), rng.uniform(-3, 3, N), np.sin(th), np.cos(th), rng.uniform(-3, 3, N)], 1)

    # -- drizzle: per frame against the same transforms per tile.  The host's share (composing 65536 N records in NumPy and their
    #    upload) is timed apart: the events bracket the whole op, so the per-tile row holds it too
    h, w = ops.drizzle_out_shape((H, W), s)
    ty, tx = -(-h // 16), -(-w // 64)
    tiles = np.broadcast_to(aff[:, None, None, :], (N, ty, tx, 6)).copy()
    print('drizzle of %d x %d x %d onto %d x %d: %d tile records' % (N, H, W, h, w, N * ty * tx))
    rows = interleaved_ms({'ops.drizzle, one transform per frame': lambda: ops.drizzle(frames, aff, s, pf),
                           'ops.drizzle, one per 16 x 64 tile (same maps)': lambda: ops.drizzle(frames, tiles, s, pf)}, p.reps)
    show(rows)
    a, b = ops.drizzle(frames, aff, s, pf), ops.drizzle(frames, tiles, s, pf)
    print('  same bits: image %s, weight %s' % (torch.equal(a['image'].view(torch.int32), b['image'].view(torch.int32)), torch.equal(a['weight'], b['weight'])))
    # the kernels alone: the parameter records prepared once, the library called directly
    import ctypes as C
    from astrophotography_amd import _lib
    lib = _lib.load()
    A = ops.drizzle_affines(aff, s)
    rec = np.concatenate([A, 0.5 * np.hypot(A[:, 0], A[:, 3])[:, None], 0.5 * np.hypot(A[:, 1], A[:, 4])[:, None], np.ones((N, 2))], 1)
    prm_f = torch.from_numpy(rec).cuda()
    prm_t = torch.from_numpy(np.broadcast_to(rec[:, None, None, :], (N, ty, tx, 10)).copy()).cuda()
    img, wgt = torch.empty((h, w), device='cuda'), torch.empty((h, w), device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel(entry, prm):
        _lib.check(entry(ptr(frames), N, H, W, None, None, ptr(prm), pf, None, 0, ptr(img), ptr(wgt), h, w, st()))
    show(interleaved_ms({'apgpu_drizzle_f32 (the kernel alone)': lambda: kernel(lib.apgpu_drizzle_f32, prm_f),
                         'apgpu_drizzle_tiles_f32 (the kernel alone)': lambda: kernel(lib.apgpu_drizzle_tiles_f32, prm_t)}, p.reps))
    del img, wgt, prm_t, a, b

    # -- resample_affine: existing code, record only
    per_tile = torch.from_numpy(np.broadcast_to(aff[:, None, None, :], (N, -(-H // 16), -(-W // 64), 6)).copy()).cuda()
    out = torch.empty((N, H, W), device='cuda')
    print('resample_affine of %d x %d x %d (existing kernels)' % (N, H, W))
    show(interleaved_ms({'resample_affine, one transform per frame': lambda: ops.resample_affine(frames, aff, out=out, weight=False),
                         'resample_affine, one per 16 x 64 tile': lambda: ops.resample_affine(frames, per_tile, out=out, weight=False)}, p.reps))
    del out, per_tile, frames
    torch.cuda.empty_cache()

    # -- tile affines for 64 frames
    x0 = y0 = (p.size - 1) / 2.0
    L = float(np.hypot(x0, y0))
    for d in (3, 5):
        maps = []
        for f in range(64):
            m = PolyMap.from_affine(rm.make_affine(0.1 * f, 1.0, shift=(f, -f), centre=(x0, y0)), d, (x0, y0), L)
            m.cx[3:] = rng.uniform(-0.5, 0.5, m.cx.size - 3)
            m.cy[3:] = rng.uniform(-0.5, 0.5, m.cy.size - 3)
            maps.append(m)
        t0 = time.perf_counter()
        tiles_d, est = ops.poly_tile_affines(maps, (p.size, p.size))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        coef = torch.from_numpy(np.stack([np.stack([m.cx, m.cy]) for m in maps])).cuda()

        def launch():
            _lib.check(lib.apgpu_poly_tile_affines(ptr(coef), 64, d, x0, y0, L, p.size, p.size, 1, 1.0, 1, ptr(tiles_d), st()))
        k = interleaved_ms({'kernel': launch}, p.reps)['kernel']
        print('poly_tile_affines, 64 frames of %d^2, degree %d: %d records, %.1f MB; kernel %.3f ms median (%.3f .. %.3f); the op with its '
              'host estimate %.1f ms wall; estimate %.2e px' % (p.size, d, tiles_d.numel() // 6, tiles_d.numel() * 8 / 1e6, k[0], k[1], k[2], 1e3 * wall, est))

    # -- register_lists
    lists, _ = make_sequence(64, 3000)
    xy_h, count_h = rm.pad_lists(lists)
    xy, count = torch.from_numpy(xy_h).cuda(), torch.from_numpy(count_h).cuda()
    for model in ('affine', 'poly3', 'affine', 'poly3'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ops.register_lists(xy, count, model=model)
        torch.cuda.synchronize()
        extra = '' if model == 'affine' else '; orders %s, rms %.3f px after %.3f px' % (sorted(set(r['order'][1:].tolist())), np.nanmedian(r['rms'][1:]), np.nanmedian(r['rms_affine'][1:]))
        print("register_lists(model='%s'), 64 frames x 3000 stars: %.1f ms wall%s" % (model, 1e3 * (time.perf_counter() - t0), extra))


if __name__ == '__main__':
    main()
