#!/usr/bin/env python3
"""Times the star finder (F6) on a synthetic 4096 x 4096 float32 field with about 3000 stars, for fwhm 3.0 and 7.9:
device time per kernel (HIP events round each entry point, median of --steps runs after --warmup), the end-to-end
ApFindStars.from_device time (host included, wall clock with a device synchronisation), and the CPU model's scipy path
(scipy.ndimage.convolve + maximum_filter, the two full-frame steps of photutils) on this host.  Reads no file.

    python tools/bench_find_stars.py [--size 4096] [--stars 3000] [--steps 10] [--warmup 3] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_field(size, nstars, seed=7):
    rng = np.random.default_rng(seed)
    img = rng.normal(300.0, 5.0, (size, size)).astype(np.float32)
    yy, xx = np.mgrid[-12:13, -12:13]
    for _ in range(nstars):
        cy, cx = rng.uniform(13, size - 13, 2)
        amp, s = rng.uniform(100, 30000), rng.uniform(1.1, 3.4)
        i, j = int(cy), int(cx)
        img[i - 12:i + 13, j - 12:j + 13] += (amp * np.exp(-((xx - (cx - j)) ** 2 + (yy - (cy - i)) ** 2) / (2 * s * s))).astype(np.float32)
    return img


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument('--size', type=int, default=4096)
    ap_.add_argument('--stars', type=int, default=3000)
    ap_.add_argument('--steps', type=int, default=10)
    ap_.add_argument('--warmup', type=int, default=3)
    ap_.add_argument('--no-cpu', action='store_true')
    a = ap_.parse_args()
    import torch
    import astrophotography_amd as ap
    from astrophotography_amd import _lib, ops
    img = make_field(a.size, a.stars)
    d = torch.from_numpy(img).cuda()
    out = dict(size=a.size, stars=a.stars, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), runs=[])
    for fwhm in (3.0, 7.9):
        k = ops.daofind_kernel(fwhm, device=d.device)
        thr = 7.0 * 5.0 * k['relerr']
        conv = ops.daofind_convolve(d, k, 300.0)
        idx, n = ops.local_peaks(conv, k['dev']['fp'], thr, border=k['R'], capacity=16384)
        rec, keep = ops.daofind_measure(d, conv, idx, k, thr, 300.0)
        sel = keep != 0
        xc, yc = rec[sel][:, 12].contiguous(), rec[sel][:, 13].contiguous()
        lst = torch.empty(16384, dtype=torch.int32, device=d.device)
        cnt = torch.empty(1, dtype=torch.int32, device=d.device)
        lib = _lib.load()

        def peaks_only():            # the entry point itself: ops.local_peaks also reads the count back and sorts
            _lib.check(lib.apgpu_local_peaks_f32(ops._ptr(conv), a.size, a.size, ops._ptr(k['dev']['fp']), 2 * k['R'] + 1, 2 * k['R'] + 1,
                                                 thr, None, k['R'], ops._ptr(lst), 16384, ops._ptr(cnt), ops._stream()))
        run = dict(fwhm=fwhm, kernel_side=2 * k['R'] + 1, candidates=n, kept=int(sel.sum()), ms={})
        run['ms']['daofind_convolve'] = timed(lambda: ops.daofind_convolve(d, k, 300.0), a.steps, a.warmup)
        run['ms']['local_peaks'] = timed(peaks_only, a.steps, a.warmup)
        run['ms']['daofind_measure'] = timed(lambda: ops.daofind_measure(d, conv, idx, k, thr, 300.0), a.steps, a.warmup)
        run['ms']['aperture_phot'] = timed(lambda: ops.aperture_photometry(d, xc, yc, fwhm), a.steps, a.warmup)
        run['ms']['sigclip_global'] = timed(lambda: ops.sigclip_global(d, sigma=3.0), a.steps, a.warmup)

        def end_to_end():
            ap.ApFindStars.from_device(d, {'EXPTIME': 1.0}, search_fwhm=fwhm, loglevel='ERROR')
            torch.cuda.synchronize()
        for _ in range(2):
            end_to_end()
        wall = []
        for _ in range(max(3, a.steps // 2)):
            t0 = time.perf_counter()
            end_to_end()
            wall.append((time.perf_counter() - t0) * 1e3)
        run['ms']['from_device_end_to_end_wall'] = (float(np.median(wall)), float(np.min(wall)))
        if not a.no_cpu:
            from scipy import ndimage
            K64 = k['K']
            t0 = time.perf_counter()
            c = ndimage.convolve(img - np.float32(300.0), K64, mode='constant', cval=0.0)
            t1 = time.perf_counter()
            mx = ndimage.maximum_filter(c, footprint=k['fp'], mode='constant', cval=0.0)
            npk = int(((c == mx) & (c > thr)).sum())
            t2 = time.perf_counter()
            run['cpu_scipy_ms'] = dict(convolve=(t1 - t0) * 1e3, maximum_filter_and_peaks=(t2 - t1) * 1e3, peaks=npk,
                                       threads=1, cpus_visible=os.cpu_count())
        out['runs'].append(run)
        print('fwhm %.1f (kernel %d x %d): %d candidates, %d kept' % (fwhm, run['kernel_side'], run['kernel_side'], n, run['kept']))
        for name, (med, mn) in run['ms'].items():
            print('    %-30s median %9.3f ms   min %9.3f ms' % (name, med, mn))
        if 'cpu_scipy_ms' in run:
            print('    cpu scipy (1 thread): convolve %.0f ms, maximum_filter + compare %.0f ms' % (
                run['cpu_scipy_ms']['convolve'], run['cpu_scipy_ms']['maximum_filter_and_peaks']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
