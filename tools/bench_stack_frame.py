#!/usr/bin/env python3
"""Times frame normalisation and weights inside the rejection rules (ops.stack_reject(scale=, offset=, weights=)) on one GPU.

Per case - 16, 32 and 64 float32 frames and 64 uint16 frames of the benchmark's synthetic raw data (synth.make_frames; no
calibration: the frame parameters exclude it), H x W = 4096 x 4096 unless --size says otherwise:

    winsorized / minmax              the call without the flag: the kernel as it was, the yardstick
    winsorized_frame / minmax_frame  the same call with random parameters near 1 / 0 / 1 (scale 1 +- 1 %, offset +- 5 ADU,
                                     weights 0.5 .. 1)

each timed with device events over --steps calls after --warmup, all four alternating.  Reported per case: milliseconds (median
and spread over the steps) and the ratio of each flagged call to its yardstick - what the map on load and the second walk over
the frames cost.  Then ops.frame_stats on --stats-frames frames against as many ops.sigclip_global calls with a host read after
each (the ops.background_weights pattern), wall clock.  One JSON line per case on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, steps, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--size', type=int, default=4096, help='image side (default 4096)')
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--cases', default='16:f32,32:f32,64:f32,64:u16', help='frames:dtype, comma separated')
    ap.add_argument('--stats-frames', type=int, default=16, help='frames of the frame_stats comparison (0: skip it)')
    ap.add_argument('--out', default=None, help='also write the JSON lines here')
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_stack_frame needs a GPU: a timing taken elsewhere says nothing')
    from astrophotography_amd import ops, synth
    H = W = args.size
    masters = synth.make_masters(H, W, config_id=2)
    nflat, _ = ops.flat_normalize(masters['flat'])
    rng = np.random.default_rng(16)
    lines = []
    for case in args.cases.split(','):
        n, dt = case.split(':')
        n = int(n)
        tdtype = torch.float32 if dt == 'f32' else torch.uint16
        frames = synth.make_frames(n, masters, nflat, config_id=2, dtype=tdtype)
        fp = dict(scale=rng.uniform(0.99, 1.01, n), offset=rng.uniform(-5.0, 5.0, n), weights=rng.uniform(0.5, 1.0, n))
        runs = {
            'winsorized': lambda: ops.stack_reject(frames, 'winsorized', outputs=('mean',)),
            'winsorized_frame': lambda: ops.stack_reject(frames, 'winsorized', outputs=('mean',), **fp),
            'minmax': lambda: ops.stack_reject(frames, 'minmax', outputs=('mean',)),
            'minmax_frame': lambda: ops.stack_reject(frames, 'minmax', outputs=('mean',), **fp),
        }
        times = {k: [] for k in runs}
        for k, fn in runs.items():                           # every shape warmed before the timed window
            _time(fn, 0, args.warmup, torch)
        for _ in range(args.steps):                          # alternating: one step of each in turn
            for k, fn in runs.items():
                times[k] += _time(fn, 1, 0, torch)
        rec = dict(frames=n, dtype=dt, size=H, kernel=ops.stack_kernel_name(n, dtype=dt, calibrated=False, rejection='winsorized'))
        for k, ms in times.items():
            rec[k] = dict(ms=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))
        for rule in ('winsorized', 'minmax'):
            rec[rule + '_frame']['vs_no_flag'] = round(rec[rule + '_frame']['ms'] / rec[rule]['ms'], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del frames
        torch.cuda.empty_cache()
    if args.stats_frames:
        n = args.stats_frames
        frames = synth.make_frames(n, masters, nflat, config_id=2, dtype=torch.float32)

        def batched():
            return ops.frame_stats(frames).cpu()

        def one_by_one():
            return [float(ops.sigclip_global(frames[i])[2].item()) for i in range(n)]

        wall = {'frame_stats': [], 'sigclip_global_with_host_reads': []}
        for fn in (batched, one_by_one):
            for _ in range(args.warmup):
                fn()
        for _ in range(args.steps):
            for k, fn in zip(wall, (batched, one_by_one)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        rec = dict(frame_stats_frames=n, size=H)
        for k, ms in wall.items():
            rec[k] = dict(ms=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))
        rec['ratio'] = round(rec['frame_stats']['ms'] / rec['sigclip_global_with_host_reads']['ms'], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
