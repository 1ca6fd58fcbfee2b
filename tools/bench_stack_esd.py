#!/usr/bin/env python3
"""Times the generalized ESD rejection rule (ops.stack_reject(method='esd')) beside the Winsorized clip on one GPU.

Per case - 16, 32, 64 and 128 float32 frames of H x W = 4096 x 4096 (--size), sky 100 ADU with noise 5 ADU from a seeded
generator on the device:

    esd / winsorized                  the data as they are ("clean")
    esd_outliers / winsorized_outliers    the same slab with +500 ADU on every pixel of two frames (every column has two outliers)

each timed with device events over --steps calls after --warmup, the four alternating in the same process.  Reported per case:
milliseconds (median and spread over the steps), ESD's ratio to Winsorized on the same slab, and the share of the time the
algorithmic bytes (N x P x 4 read + 4 P written) need at 8 TB/s.  With --model-columns K the NumPy model runs on K columns of the
same slab and reports what the kernel's trip count is made of: the steps a column allows (K), and the share of columns that lose a
value.  One JSON line per case on stdout (and in --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


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
    ap.add_argument('--frames', default='16,32,64,128', help='frame counts, comma separated')
    ap.add_argument('--outliers', type=float, default=0.3, help='esd_outliers')
    ap.add_argument('--model-columns', type=int, default=0, help='columns of each slab the NumPy model runs on')
    ap.add_argument('--out', default=None, help='also write the JSON lines here')
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_stack_esd needs a GPU: a timing taken elsewhere says nothing')
    from astrophotography_amd import ops
    H = W = args.size
    P = H * W
    lines = []
    for n in (int(v) for v in args.frames.split(',')):
        gen = torch.Generator(device='cuda').manual_seed(1000 + n)
        clean = torch.empty((n, H, W), dtype=torch.float32, device='cuda').normal_(100.0, 5.0, generator=gen)
        dirty = clean.clone()
        for f in (1, n // 2):
            dirty[f] += 500.0
        table = ops.esd_lambda(n, args.outliers, 0.05)       # computed once, outside the timed window
        kw = dict(esd_outliers=args.outliers, esd_table=table, outputs=('mean',))
        runs = {
            'winsorized': lambda: ops.stack_reject(clean, 'winsorized', outputs=('mean',)),
            'esd': lambda: ops.stack_reject(clean, 'esd', **kw),
            'winsorized_outliers': lambda: ops.stack_reject(dirty, 'winsorized', outputs=('mean',)),
            'esd_outliers': lambda: ops.stack_reject(dirty, 'esd', **kw),
        }
        times = {k: [] for k in runs}
        for k, fn in runs.items():                           # every shape warmed before the timed window
            _time(fn, 0, args.warmup, torch)
        for _ in range(args.steps):                          # alternating: one step of each in turn
            for k, fn in runs.items():
                times[k] += _time(fn, 1, 0, torch)
        floor_ms = (n * P * 4 + 4 * P) / HBM_BYTES_PER_S * 1e3
        rec = dict(frames=n, size=H, esd_outliers=args.outliers, steps_allowed=int(table.shape[1]), bytes_floor_ms=round(floor_ms, 4),
                   kernel=dict(esd=ops.stack_kernel_name(n, calibrated=False, rejection='esd'),
                               winsorized=ops.stack_kernel_name(n, calibrated=False, rejection='winsorized')))
        for k, ms in times.items():
            med = float(np.median(ms))
            rec[k] = dict(ms=round(med, 4), min=round(min(ms), 4), max=round(max(ms), 4), share_of_bytes_floor=round(floor_ms / med, 4))
        rec['esd_vs_winsorized'] = round(rec['esd']['ms'] / rec['winsorized']['ms'], 3)
        rec['esd_vs_winsorized_outliers'] = round(rec['esd_outliers']['ms'] / rec['winsorized_outliers']['ms'], 3)
        if args.model_columns:
            from tests import stack_esd_model as model
            k = args.model_columns
            sel = torch.arange(0, P, max(1, P // k), device='cuda')[:k]
            for name, slab in (('esd', clean), ('esd_outliers', dirty)):
                m = model.esd(slab.reshape(n, -1)[:, sel].cpu().numpy(), table, args.outliers, 1.5)
                rec[name]['model'] = dict(columns=int(sel.numel()), steps_mean=float(m['steps'].mean()), steps_max=int(m['steps'].max()),
                                          columns_losing_a_value=float((m['count'] < n).mean()),
                                          rejected=float(1.0 - m['count'].sum() / (n * sel.numel())))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del clean, dirty
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
