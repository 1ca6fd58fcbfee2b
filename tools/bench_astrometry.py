#!/usr/bin/env python3
"""F21 timing: the two kernels of csrc/astrometry.hip on catalogues of 10^6 and 10^7 stars in a 5 degree cone with the search cells of a
4096 x 4096 frame, and ops.solve_field end to end on 3000 image stars.

  sky_project  33 B per star (ra, dec read; xi, eta, keep written)
  cell_select  per cell 16 B for every star the walk reads: all n where the cell does not fill, else up to the trip (1024 stars) that
               holds its capacity-th star - counted from the result.  With capacity 512 every cell of a dense catalogue fills early (a
               launch's latency); with capacity 65536 the cells that do not fill read the whole list (only those are counted)
  solve_field  wall time, and where it goes: each ops function it calls is timed (with a device synchronisation) in one extra run

Device time by HIP events (one warm-up call, then the median, minimum and maximum of --reps calls); GB/s = algorithmic bytes / time
beside the 8 TB/s HBM peak; and the time tests/astrometry_model.py (NumPy) takes for the same step on this host.

    python tools/bench_astrometry.py [--reps 20] [--stars 1000000 10000000]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0
CENTRE, CONE, SIZE, SCALE, RATIO, RADIUS = (83.6, 22.0), 5.0, 4096, 1.0, 1.3, 1.0


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


def row(label, ms, nbytes, host_s=None):
    med, mn, mx = ms
    gbs = nbytes / med / 1e6
    tail = '' if host_s is None else '  NumPy model %.3f s' % host_s
    print('  %-52s %8.3f ms median (%7.3f .. %7.3f)  %7.0f GB/s  %4.1f %% of peak%s' % (label, med, mn, mx, gbs, 100.0 * gbs / PEAK_GBS, tail))


def catalogue(n, seed):
    rng = np.random.default_rng(seed)
    r, th = CONE * np.sqrt(rng.uniform(size=n)), rng.uniform(0.0, 2.0 * np.pi, size=n)
    dec = CENTRE[1] + r * np.sin(th)
    ra = CENTRE[0] + r * np.cos(th) / np.cos(np.deg2rad(dec))
    return dict(ra=ra, dec=dec, mag=16.0 + np.log10(rng.uniform(size=n)) / 0.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--stars', type=int, nargs='+', default=[1000000, 10000000])
    p = ap.parse_args()
    import torch
    from astrophotography_amd import ops
    from tests import astrometry_model as am
    print('F21 astrometry; device %s; %d repetitions after one warm-up call' % (torch.cuda.get_device_name(0), p.reps))
    shape = (SIZE, SIZE)
    cells, cos_rc = ops.astrometry_cells(shape, SCALE, RATIO, RADIUS)
    print('%d cells of a %d x %d frame at %.1f arcsec / px, ratio %.1f, radius %.1f deg; capacity 512' % (len(cells), SIZE, SIZE, SCALE, RATIO, RADIUS))
    for n in p.stars:
        cat = catalogue(n, n % 97)
        ra, dec, mag = (torch.from_numpy(cat[k]).cuda() for k in ('ra', 'dec', 'mag'))
        t0 = time.perf_counter()
        mxi, meta, mkeep = am.project(cat['ra'], cat['dec'], CENTRE[0], CENTRE[1], cos_rc)
        host_project = time.perf_counter() - t0
        row('sky_project, %d stars (33 B a star)' % n, device_ms(lambda: ops.sky_project(ra, dec, CENTRE, cos_rc), p.reps), 33 * n, host_project)
        xi, eta, keep = ops.sky_project(ra, dec, CENTRE, cos_rc)
        kept = torch.nonzero(keep).reshape(-1)
        kept = kept[torch.sort(mag[kept], stable=True)[1]]
        X, Y = (-xi[kept]) * 3600.0 / SCALE, eta[kept] * 3600.0 / SCALE
        m = int(kept.numel())
        idx, count, inside = ops.cell_select(X, Y, cells, 512)
        last = idx[:, -1].cpu().numpy().astype(np.int64)
        read = np.where(last >= 0, np.minimum((last // 1024 + 1) * 1024, m), m)
        t0 = time.perf_counter()
        am.cell_select(X.cpu().numpy(), Y.cpu().numpy(), cells, 512)
        host_select = time.perf_counter() - t0
        row('cell_select, %d kept stars, %d cells (%d full)' % (m, len(cells), int((last >= 0).sum())),
            device_ms(lambda: ops.cell_select(X, Y, cells, 512), p.reps), 16 * int(read.sum()), host_select)
        big = ops.cell_select(X, Y, cells, 65536)[2].cpu().numpy()
        walked = int((big <= 65536).sum())
        row('cell_select, capacity 65536: %d cells read all stars' % walked, device_ms(lambda: ops.cell_select(X, Y, cells, 65536), p.reps),
            16 * m * walked)
    # end to end: a 4096 x 4096 frame seen in the first catalogue, its 3000 brightest stars
    cat = catalogue(p.stars[0], p.stars[0] % 97)
    truth = am.planted_wcs(am.unproject(0.3, -0.2, CENTRE[0], CENTRE[1]), shape, SCALE * 1.07, 33.0, False)
    xy, _ = am.observe(5, cat, truth, shape, spurious=0.002)        # (observe() draws spurious magnitudes uniformly: 0.2 % is a dozen among the 40 brightest)
    xy = xy[:3000]
    args = (xy, shape, cat, CENTRE, SCALE, RATIO, RADIUS)
    dev_cat = {k: torch.from_numpy(v).cuda() for k, v in cat.items()}
    r = ops.solve_field(xy, shape, dev_cat, *args[3:])
    torch.cuda.synchronize()
    walls = []
    for _ in range(max(3, p.reps // 4)):
        t0 = time.perf_counter()
        r = ops.solve_field(xy, shape, dev_cat, *args[3:])
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    corner = am.corner_error(r['wcs'], truth, shape) if r['wcs'] is not None else float('nan')
    print('  %-52s %8.1f ms median wall (%7.1f .. %7.1f); status %d, %d of %d stars matched, rms %.3f px, corner error %.3f px'
          % ('solve_field, %d image stars, catalogue on the device' % len(xy), float(np.median(walls)), min(walls), max(walls), r['status'],
             r['n_matched'], len(xy), r['rms'], corner))
    spent, depth = {}, [0]

    def timed(name):
        fn = getattr(ops, name)

        def wrapper(*a, **k):
            if depth[0]:                                     # called by a step that is being timed: part of that step
                return fn(*a, **k)
            depth[0] += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                torch.cuda.synchronize()
                spent[name] = spent.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
                depth[0] -= 1
        setattr(ops, name, wrapper)
        return fn
    notes = (('sky_project', 'the catalogue about the hint'), ('cell_select', 'the cells'), ('triangle_build', 'frame 0 and every cell'),
             ('triangle_vote', 'frame 0 against every cell'), ('register_lists', 'the candidates: votes, seeds, neighbour rounds, fits'),
             ('tan_fit', 'the first fit, host'), ('_solve_rematch', 'the rounds on the whole catalogue: host projection, nearest_match, fits'))
    saved = {n: timed(n) for n, _ in notes}
    t0 = time.perf_counter()
    ops.solve_field(xy, shape, dev_cat, *args[3:])
    torch.cuda.synchronize()
    total = 1e3 * (time.perf_counter() - t0)
    for n, fn in saved.items():
        setattr(ops, n, fn)
    print('  one run with every step synchronised: %.1f ms' % total)
    for n, note in notes:
        print('    %-18s %8.1f ms  (%s)' % (n, spent.get(n, 0.0), note))
    print('    %-18s %8.1f ms  (the finite test, the sort by magnitude, the gathers, the read-backs)' % ('the rest', total - sum(spent.values())))
    t0 = time.perf_counter()
    out, _ = am.solve_field(*args)
    print('  NumPy model of the same solve on this host: %.1f s, status %d, %d matched' % (time.perf_counter() - t0, out['status'], out['n_matched']))


if __name__ == '__main__':
    main()
