#!/usr/bin/env python3
"""F23 timing: the two kernels of csrc/subtract.hip and ApSubtract.subtract end to end on a 4096 x 4096 pair.

  stamps   100 and 400 stamps of 31 x 31 with the default basis (49 functions, radius 10): one workgroup a stamp
  apply    radius 5, 10, 15 and kernel degree 0, 2, 3 (1, 6, 10 composite kernels), beside
             the VALU floor   2 NT (2 r + 1)^2 float32 operations per pixel (a multiply and an add per tap and kernel: no fused
                              multiply-add by contract) at 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz - derived, not measured
             the bytes        4 B read of each image and 4 B written per pixel at 8 TB/s
  subtract ApSubtract.subtract with a given star list (the host's selection, solve and transfers included)

Device time by HIP events (one warm-up call, then the median, minimum and maximum of --reps calls).  The kernel rows time the C
entry points themselves on buffers that are uploaded and allocated once, so that no upload, allocation or argument check of the
ops layer lies between the events; the end-to-end row is the wall time of everything.

    python tools/bench_subtract.py [--reps 10] [--size 4096]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_OPS_PER_S = 256 * 4 * 32 * 2.4e9
HBM_BYTES_PER_S = 8e12


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


def wall_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def row(label, ms, note=''):
    print('  %-58s %9.3f ms median (%9.3f .. %9.3f)  %s' % ((label,) + tuple(ms) + (note,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--size', type=int, default=4096)
    p = ap.parse_args()
    import torch
    from astrophotography_amd import _lib, ops
    from astrophotography_amd.core.ApSubtract import ApSubtract
    N = p.size
    rng = np.random.default_rng(0)
    side = 20
    xs, ys = np.meshgrid((np.arange(side) + 0.5) * N / side, (np.arange(side) + 0.5) * N / side)
    x, y = xs.ravel() + rng.uniform(-3, 3, side * side), ys.ravel() + rng.uniform(-3, 3, side * side)
    peak = np.exp(rng.uniform(np.log(800.0), np.log(8000.0), side * side))
    T = torch.full((N, N), 100.0, device='cuda') + 2.0 * torch.randn((N, N), device='cuda')
    yy, xx = np.mgrid[-9:10, -9:10].astype(np.float64)
    for k in range(len(x)):                                          # round Gaussian stars, sigma 1.3, on the device planes
        cx, cy = int(round(x[k])), int(round(y[k]))
        g = peak[k] * np.exp(-((xx - (x[k] - cx)) ** 2 + (yy - (y[k] - cy)) ** 2) / (2 * 1.3 ** 2))
        T[cy - 9:cy + 10, cx - 9:cx + 10] += torch.from_numpy(g.astype(np.float32)).cuda()
    I = 0.8 * ops.gauss_blur(T, 1.0) + 30.0 + 5.0 * torch.randn((N, N), device='cuda')
    print('F23 optimal image subtraction on %d x %d, %d stars (MI355X; device time by HIP events, %d repetitions)' % (N, N, len(x), p.reps))
    basis = ops.kernel_basis()
    cen = np.stack([np.rint(x), np.rint(y)], 1).astype(np.int64)
    print(' stamps kernel (default basis: %d functions, radius %d; stamps of 31 x 31)' % (basis['nb'], basis['radius']))
    lib, st = _lib.load(), ops._stream
    H = W = N
    filters = torch.from_numpy(basis['filters']).cuda()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    brow, bcol, beven, bscale = basis['row'], basis['col'], basis['even'], basis['scale']
    for S in (100, 400):
        cd = torch.from_numpy(np.ascontiguousarray(cen[:S].astype(np.int32))).cuda()
        gram = torch.empty((S, basis['nb'] + 2, basis['nb'] + 2), dtype=torch.float64, device='cuda')
        status, count = torch.empty(S, dtype=torch.int32, device='cuda'), torch.empty(S, dtype=torch.int32, device='cuda')

        def stamps():
            _lib.check(lib.apgpu_subtract_stamps_f32(ops._ptr(T), ops._ptr(I), None, H, W, ops._ptr(cd), S, 15, basis['radius'], ops._ptr(filters),
                                                     int(filters.shape[0]), brow.ctypes.data_as(ip), bcol.ctypes.data_as(ip), bscale.ctypes.data_as(dp),
                                                     beven.ctypes.data_as(ip), basis['nb'], 0.0, 0.0, ops._ptr(gram), ops._ptr(status), ops._ptr(count), st()))
        ms = device_ms(stamps, p.reps)
        row('%d stamps (%d accepted)' % (S, int((status == 0).sum())), ms)
    print(' apply kernel')
    byte_ms = 1e3 * 3 * 4 * N * N / HBM_BYTES_PER_S
    diff = torch.empty_like(T)
    bg = np.zeros(1)
    for r in (5, 10, 15):
        for deg in (0, 2, 3):
            nt = (deg + 1) * (deg + 2) // 2
            kd = torch.from_numpy((rng.standard_normal((nt, 2 * r + 1, 2 * r + 1)) / (2 * r + 1) ** 2).astype(np.float32)).cuda()
            floor = 1e3 * 2 * nt * (2 * r + 1) ** 2 * N * N / VALU_OPS_PER_S

            def apply():
                _lib.check(lib.apgpu_subtract_apply_f32(ops._ptr(T), ops._ptr(I), H, W, ops._ptr(kd), r, deg, bg.ctypes.data_as(dp), 0, 0, 1.0,
                                                        ops._ptr(diff), None, st()))
            ms = device_ms(apply, p.reps)
            row('radius %2d, degree %d (%2d kernels)' % (r, deg, nt), ms,
                'VALU floor %.3f ms (%.0f %% of it reached), bytes %.3f ms' % (floor, 100.0 * floor / ms[0], byte_ms))
    print(' end to end')
    sub = ApSubtract(loglevel='ERROR')
    stars = np.stack([x, y, peak * 2 * np.pi * 1.3 ** 2, peak], 1)
    row('ApSubtract.subtract (star list given, defaults)', wall_ms(lambda: sub.subtract(I, T, stars=stars), max(3, p.reps // 3)), 'wall time')
    rep = sub.subtract(I, T, stars=stars)['report']
    print('  scale %.5f, %d stamps used, %d rejected, %d refused, condition number %.3g' % (rep['scale'], rep['used'], rep['rejected'], rep['refused'], rep['cond']))


if __name__ == '__main__':
    main()
