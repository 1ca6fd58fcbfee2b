#!/usr/bin/env python3
"""F5 ApAutoBadcols on the device: device-event times (warm-up first) and the HBM roofline of the algorithmic bytes
(each axis median reads the image once: 2 N H W sizeof bytes).
    python tools/bench_autobadcol.py [--reps 10] [--quick]"""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import astrophotography_amd as apmod
from astrophotography_amd import ops

HBM_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--quick', action='store_true', help='one frame and 8-frame slabs only (for a profiler run)')
a = ap.parse_args()


def t(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


g = torch.Generator(device='cuda').manual_seed(5)
results = []


def report(what, ms, nbytes):
    tbs = nbytes / (ms * 1e-3) / 1e12
    r = dict(what=what, ms=round(ms, 4), algorithmic_bytes=nbytes, tb_per_s=round(tbs, 3), hbm_fraction=round(tbs / HBM_TBS, 3))
    results.append(r)
    print('%-58s %9.3f ms  %7.3f TB/s  %.3f of %.0f TB/s' % (what, ms, tbs, tbs / HBM_TBS, HBM_TBS), flush=True)


frame = 1000.0 + 15.0 * torch.randn((4096, 4096), generator=g, device='cuda')
frame[:, 1234] += 300.0
frame_host = frame.cpu().numpy()
ab = apmod.ApAutoBadcols('WARNING')
report('ApAutoBadcols.process, 1 x 4096^2 f32, host array in', t(lambda: ab.process(frame_host), a.reps), 2 * frame.numel() * 4)
report('ApAutoBadcols.process, 1 x 4096^2 f32, device tensor in', t(lambda: ab.process(frame), a.reps), 2 * frame.numel() * 4)
report('ops.auto_badcols, 1 x 4096^2 f32', t(lambda: ops.auto_badcols(frame), a.reps), 2 * frame.numel() * 4)
report('  axis_nanmedian axis 0 (columns), 1 x 4096^2 f32', t(lambda: ops.axis_nanmedian(frame, 0), a.reps), frame.numel() * 4)
report('  axis_nanmedian axis 1 (rows), 1 x 4096^2 f32', t(lambda: ops.axis_nanmedian(frame, 1), a.reps), frame.numel() * 4)
med = ops.axis_nanmedian(frame, 0)
report('  sliding_clipped_stats, 4096 f32, window 11', t(lambda: ops.sliding_clipped_stats(med, 11), a.reps), med.numel() * 4)
med64 = med.double()
report('  sliding_clipped_stats, 4096 f64, window 11', t(lambda: ops.sliding_clipped_stats(med64, 11), a.reps), med.numel() * 8)
report('  sliding_clipped_stats, 4096 f32, window 301', t(lambda: ops.sliding_clipped_stats(med, 301), a.reps), med.numel() * 4)
report('  sliding_clipped_stats, 4096 f64, window 301', t(lambda: ops.sliding_clipped_stats(med64, 301), a.reps), med.numel() * 8)
del frame

N = 8 if a.quick else 64
slab = 1000.0 + 15.0 * torch.randn((N, 4096, 4096), generator=g, device='cuda')
report('ops.auto_badcols, %d x 4096^2 f32' % N, t(lambda: ops.auto_badcols(slab), max(2, a.reps // 2)), 2 * slab.numel() * 4)
report('  axis_nanmedian axis 0, %d x 4096^2 f32' % N, t(lambda: ops.axis_nanmedian(slab, 0), max(2, a.reps // 2)), slab.numel() * 4)
report('  axis_nanmedian axis 1, %d x 4096^2 f32' % N, t(lambda: ops.axis_nanmedian(slab, 1), max(2, a.reps // 2)), slab.numel() * 4)
del slab
torch.cuda.empty_cache()
u16 = torch.randint(0, 65536, (N, 4176, 6248), generator=g, device='cuda', dtype=torch.int32).to(torch.int16).view(torch.uint16)
report('ops.auto_badcols, %d x 6248x4176 u16 (C4 geometry)' % N, t(lambda: ops.auto_badcols(u16), max(2, a.reps // 2)),
       2 * u16.numel() * 2)
print(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results)))
