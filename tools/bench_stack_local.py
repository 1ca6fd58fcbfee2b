#!/usr/bin/env python3
"""Times the local normalisation inside the rejection rules (ops.stack_reject(offset=mesh, box=)) on one GPU (F17).

Per case - 16, 32 and 64 float32 frames and 64 uint16 frames of the benchmark's synthetic raw data (synth.make_frames; no
calibration: the flag excludes it), H x W = 4096 x 4096 unless --size says otherwise - and per box size (128 and 256 pixels):

    winsorized_frame / minmax_frame  the call with APGPU_STACK_FRAME_PARAMS and random parameters near 1 / 0 / 1 (scale 1 +- 1 %,
                                     offset +- 5 ADU, weights 0.5 .. 1): the parent commit's kernel, unchanged - the yardstick
    winsorized_local / minmax_local  the same call with scale and offset MESHES of the same spread, one value per box
    *_local_add                      ... without a scale mesh (the additive mode: four loads and three lerps less per value)

each timed with device events over --steps calls after --warmup, all alternating.  Reported per case: milliseconds (median and
spread over the steps) and the ratio of each local call to its yardstick - what the mesh loads and the lerps cost, on load and
again in the weighted walk.  Then ops.local_stats on --stats-frames frames against as many ops.box_clipped_stats calls with a host
read after each, wall clock, per box size.  One JSON line per case on stdout (and in --out)."""
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
    ap.add_argument('--boxes', default='128,256', help='box sides in pixels, comma separated')
    ap.add_argument('--stats-frames', type=int, default=16, help='frames of the local_stats comparison (0: skip it)')
    ap.add_argument('--out', default=None, help='also write the JSON lines here')
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_stack_local needs a GPU: a timing taken elsewhere says nothing')
    from astrophotography_amd import ops, synth
    H = W = args.size
    boxes = [int(b) for b in args.boxes.split(',')]
    masters = synth.make_masters(H, W, config_id=2)
    nflat, _ = ops.flat_normalize(masters['flat'])
    rng = np.random.default_rng(17)
    lines = []
    for case in args.cases.split(','):
        n, dt = case.split(':')
        n = int(n)
        tdtype = torch.float32 if dt == 'f32' else torch.uint16
        frames = synth.make_frames(n, masters, nflat, config_id=2, dtype=tdtype)
        w = rng.uniform(0.5, 1.0, n)
        fp = dict(scale=rng.uniform(0.99, 1.01, n), offset=rng.uniform(-5.0, 5.0, n), weights=w)
        for box in boxes:
            ny, nx = -(-H // box), -(-W // box)
            A, B = rng.uniform(0.99, 1.01, (n, ny, nx)), rng.uniform(-5.0, 5.0, (n, ny, nx))
            runs = {}
            for rule in ('winsorized', 'minmax'):
                runs[rule + '_frame'] = lambda rule=rule: ops.stack_reject(frames, rule, outputs=('mean',), **fp)
                runs[rule + '_local'] = lambda rule=rule: ops.stack_reject(frames, rule, outputs=('mean',), scale=A, offset=B, weights=w, box=box)
                runs[rule + '_local_add'] = lambda rule=rule: ops.stack_reject(frames, rule, outputs=('mean',), offset=B, weights=w, box=box)
            times = {k: [] for k in runs}
            for k, fn in runs.items():                       # every shape warmed before the timed window
                _time(fn, 0, args.warmup, torch)
            for _ in range(args.steps):                      # alternating: one step of each in turn
                for k, fn in runs.items():
                    times[k] += _time(fn, 1, 0, torch)
            rec = dict(frames=n, dtype=dt, size=H, box=box, mesh=[ny, nx])
            for k, ms in times.items():
                rec[k] = dict(ms=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))
            for rule in ('winsorized', 'minmax'):
                for k in ('_local', '_local_add'):
                    rec[rule + k]['vs_frame_flag'] = round(rec[rule + k]['ms'] / rec[rule + '_frame']['ms'], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del frames
        torch.cuda.empty_cache()
    if args.stats_frames:
        n = args.stats_frames
        frames = synth.make_frames(n, masters, nflat, config_id=2, dtype=torch.float32)
        for box in boxes:
            def batched():
                return ops.local_stats(frames, box).cpu()

            def one_by_one():
                return [ops.box_clipped_stats(frames[i], None, box, box).cpu() for i in range(n)]

            wall = {'local_stats': [], 'box_clipped_stats_with_host_reads': []}
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
            rec = dict(local_stats_frames=n, size=H, box=box)
            for k, ms in wall.items():
                rec[k] = dict(ms=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))
            rec['ratio'] = round(rec['local_stats']['ms'] / rec['box_clipped_stats_with_host_reads']['ms'], 3)
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
