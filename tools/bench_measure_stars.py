#!/usr/bin/env python3
"""Times the Gaussian PSF fits (F7) on a synthetic 4096 x 4096 float32 field of Poisson counts: the fit kernel alone for 25 and
for 3000 stars (HIP events round ops.gauss2d_fit's entry point, median of --steps runs after --warmup; the call includes the
small host <-> device copies of the boxes and the records) and ApFindStars.measure_fwhm(None) end to end (wall clock with a
device synchronisation).  Reads no file.

    python tools/bench_measure_stars.py [--size 4096] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_field(size, nstars, fwhm=3.4, seed=11):
    rng = np.random.default_rng(seed)
    img = np.full((size, size), 300.0)
    s = fwhm / 2.35482
    step = int(size / math_ceil_sqrt(nstars))
    yy, xx = np.mgrid[-15:16, -15:16]
    xs, ys, amps = [], [], []
    for k in range(nstars):
        gy, gx = divmod(k, math_ceil_sqrt(nstars))
        cy = gy * step + step / 2 + rng.uniform(-1, 1)
        cx = gx * step + step / 2 + rng.uniform(-1, 1)
        amp = rng.uniform(800, 30000)
        i, j = int(cy), int(cx)
        img[i - 15:i + 16, j - 15:j + 16] += amp * np.exp(-((xx - (cx - j)) ** 2 + (yy - (cy - i)) ** 2) / (2 * s * s))
        xs.append(cx), ys.append(cy), amps.append(amp)
    return rng.poisson(img).astype(np.float32), np.array(xs), np.array(ys), np.array(amps)


def math_ceil_sqrt(n):
    r = int(np.sqrt(n))
    return r if r * r >= n else r + 1


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument('--size', type=int, default=4096)
    ap_.add_argument('--steps', type=int, default=10)
    ap_.add_argument('--warmup', type=int, default=3)
    a = ap_.parse_args()
    import torch
    import astrophotography_amd as ap
    from astrophotography_amd import ops
    out = dict(size=a.size, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), runs=[])
    for nstars in (25, 3000):
        img, xs, ys, amps = make_field(a.size, nstars)
        d = torch.from_numpy(img).cuda()
        bg = np.full(nstars, 300.0)
        fit = lambda: ops.gauss2d_fit(d, xs, ys, amps, bg, 3.0)
        for _ in range(a.warmup):
            r = fit()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fit()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        run = dict(stars=nstars, box_width=18, fit_ok=int(r['fit_ok'].sum()), iterations_mean=[float(x) for x in r['niter'].mean(axis=0)],
                   gauss2d_fit_ms_median=float(np.median(ms)), gauss2d_fit_ms_min=float(np.min(ms)),
                   median_fwhm=float(np.median(np.r_[r['fwhm_x'], r['fwhm_y']])))
        # end to end: ApFindStars on the frame, then measure_fwhm (selection on the host, 25 fits on the device)
        obj = ap.ApFindStars.from_device(d, {'EXPOSURE': 30.0}, search_fwhm=3.0)
        wall = []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = obj.measure_fwhm(None)
            torch.cuda.synchronize()
            if k >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
        run.update(sources_in_full_list=int(len(obj._full_srclist['id'])), measure_fwhm_ms_median=float(np.median(wall)),
                   measure_fwhm_ms_min=float(np.min(wall)), measure_fwhm_result=[float(res[0]), float(res[1]), int(res[2])])
        out['runs'].append(run)
        print('%5d stars: gauss2d_fit %.3f ms (min %.3f), %d ok, mean iterations %s; measure_fwhm end to end %.2f ms (%d sources)' % (
            nstars, run['gauss2d_fit_ms_median'], run['gauss2d_fit_ms_min'], run['fit_ok'],
            ['%.1f' % x for x in run['iterations_mean']], run['measure_fwhm_ms_median'], run['sources_in_full_list']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
