#!/usr/bin/env python3
"""F22 timing: the five kernels of csrc/epsf.hip and ops.epsf_build / ApEmpiricalPsf.photometry end to end on a rendered 4096 x 4096
field of 3000 stars, at oversampling 2 and 4 and stamp radius 12 and 24.

  accumulate  500 stars (the build's default), the default clip: per node up to 12 passes over the stars, an interpolation each
  update      add + 5 x 5 smoothing over the grid; shift: one interpolation per node
  fit         3000 stars, r_fit 4 (49 pixels a star), one wavefront a star; and the second-pass form
  render      3000 stars into the model and the residual plane: 2 x 4 B per pixel written, 4 B read, and the stamps
  epsf_build  wall time of the whole build (8 rounds at most, the host's share included); photometry(passes=2) likewise

Device time by HIP events (one warm-up call, then the median, minimum and maximum of --reps calls).

    python tools/bench_epsf.py [--reps 10] [--size 4096] [--stars 3000]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def planted_grid(o, R, r_fit, fwhm=3.2):
    """An elliptical Moffat (beta 2.5, axis ratio 0.8, rotated 30 degrees) plus a faint offset Gaussian lobe on the grid, moved so that
    its centre of mass within r_fit is the origin, sum / o^2 = 1: float64 [G, G]."""
    from astrophotography_amd import ops
    G = 2 * o * R + 1
    off = (np.arange(G) - o * R) / float(o)
    alpha, c, s = fwhm / (2.0 * np.sqrt(2.0 ** 0.4 - 1.0)), np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))

    def psf(dx, dy):
        a, b = c * dx + s * dy, -s * dx + c * dy
        return (1.0 + (a * a + (b / 0.8) ** 2) / alpha ** 2) ** -2.5 + 0.04 * np.exp(-0.5 * ((dx - 2.2) ** 2 + (dy + 1.4) ** 2) / 1.21)
    centre = np.zeros(2)
    for _ in range(60):
        centre += ops.epsf_centroid(psf(off[None, :] + centre[0], off[:, None] + centre[1]), o, r_fit)
    g = psf(off[None, :] + centre[0], off[:, None] + centre[1])
    return g / (g.sum() / (o * o))


def field(size, n, o, R, seed=5):
    """n stars at least 2 R + 6 apart under the planted PSF, rendered on the device."""
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(seed)
    truth = planted_grid(o, R, 4.0)
    cell = size / np.ceil(np.sqrt(n))
    gy, gx = np.divmod(np.arange(n), int(np.ceil(np.sqrt(n))))
    slack = max(cell - (2 * R + 6), 0.0)
    x = (gx + 0.5) * cell + rng.uniform(-0.5, 0.5, n) * slack
    y = (gy + 0.5) * cell + rng.uniform(-0.5, 0.5, n) * slack
    flux = 10.0 ** rng.uniform(3.7, 5.0, n)
    E = torch.from_numpy(truth.astype(np.float32)).cuda()
    model, _ = ops.epsf_render(None, np.stack([flux, x, y], axis=1), E, o, shape=(size, size), residual=False)
    image = model + 100.0 + 5.0 * torch.randn((size, size), device='cuda', generator=torch.Generator('cuda').manual_seed(seed))
    return image.contiguous(), x, y, flux, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--stars', type=int, default=3000)
    p = ap.parse_args()
    import torch
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApEmpiricalPsf import ApEmpiricalPsf
    print('F22 empirical PSF; device %s; %d repetitions after one warm-up call; %d x %d field, %d stars' % (
        torch.cuda.get_device_name(0), p.reps, p.size, p.size, p.stars))
    rng = np.random.default_rng(1)
    for o in (2, 4):
        for R in (12, 24):
            image, x, y, flux, truth = field(p.size, p.stars, o, R)
            G = 2 * o * R + 1
            n = len(x)
            x0, y0 = x + rng.uniform(-0.15, 0.15, n), y + rng.uniform(-0.15, 0.15, n)
            print('oversampling %d, radius %d: grid %d x %d (%d KiB)' % (o, R, G, G, G * G * 4 // 1024))
            E = torch.from_numpy(truth.astype(np.float32)).cuda()
            order = np.argsort(-flux)[:500]                                  # (all of them when there are fewer)
            s500 = torch.from_numpy(np.stack([flux[order], x0[order], y0[order], np.full(len(order), 100.0)], axis=1)).cuda()
            row('accumulate, %d stars, %d nodes' % (len(order), G * G), device_ms(lambda: ops.epsf_accumulate(image, s500, E, o), p.reps))
            mean, count = ops.epsf_accumulate(image, s500, E, o)
            taps = ops.epsf_smoothing_taps('quartic')
            row('update (add + smooth)', device_ms(lambda: ops.epsf_update(E, mean, count, o, taps, recentre=False, normalise=False), p.reps))
            row('shift', device_ms(lambda: ops.epsf_shift(E, o, 0.013, -0.021), p.reps))
            init = torch.from_numpy(np.stack([0.92 * flux, x0, y0, np.full(n, 100.0)], axis=1)).cuda()
            row('fit, %d stars, r_fit 4' % n, device_ms(lambda: ops.epsf_fit(image, init, E, o, 4.0), p.reps))
            rec = ops.epsf_fit(image, init, E, o, 4.0)
            iters = rec[:, 6].cpu().numpy()
            print('      (%d of %d ok, %.1f iterations a star on average, %d at most)' % (int(rec[:, 7].sum()), n, iters.mean(), iters.max()))
            row('fit with the noise model and the sky', device_ms(lambda: ops.epsf_fit(image, init, E, o, 4.0, True, 1.5, 5.0), p.reps))
            stars3 = rec[:, :3].contiguous()
            lists = ops.epsf_tile_lists(rec[:, 1].cpu().numpy(), rec[:, 2].cpu().numpy(), R, image.shape)
            ms = device_ms(lambda: ops.epsf_render(image, stars3, E, o, lists=lists), p.reps)
            row('render, model and residual, %d tile entries' % int(lists[1].numel()), ms, '%.0f GB/s of plane traffic' % (12.0 * p.size * p.size / ms[0] / 1e6))
            _, resid = ops.epsf_render(image, stars3, E, o, lists=lists, model=False)
            row('fit, second-pass form', device_ms(lambda: ops.epsf_fit(resid, rec[:, :4].contiguous(), E, o, 4.0, prev=stars3), p.reps))
            t0 = time.perf_counter()
            ops.epsf_tile_lists(rec[:, 1].cpu().numpy(), rec[:, 2].cpu().numpy(), R, image.shape)
            print('  %-58s %9.3f ms (host)' % ('tile lists', 1e3 * (time.perf_counter() - t0)))
            reps = max(2, p.reps // 5)
            sky = np.full(n, 100.0)
            built = {}

            def build():
                built.update(ops.epsf_build(image, x0, y0, 0.92 * flux, sky, o=o, R=R, r_fit=4.0))
            row('epsf_build, wall', wall_ms(build, reps))
            err = float(np.abs(built['epsf'].cpu().numpy().astype(np.float64) - truth).max() / truth.max())
            print('      (%d stars, %d rounds, last change %.2e, error against the planted PSF %.2e of the peak)' % (
                len(built['index']), built['niter'], built['change'][-1], err))
            ep = ApEmpiricalPsf(loglevel='ERROR', oversampling=o, radius=R, fit_radius=4.0)
            stars = dict(xcenter=x0, ycenter=y0, aperture_sum=0.92 * flux, bgmed_per_pix=sky)
            row('photometry(passes=2), wall', wall_ms(lambda: ep.photometry(image, stars, passes=2, epsf=built['epsf']), reps))


if __name__ == '__main__':
    main()
