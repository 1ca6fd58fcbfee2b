"""The headline stack (fused calibrate + 3-sigma clipped mean, 64 x 4096^2 float32) with ONE exposure ratio for all frames and
with a ratio that differs per frame: the fast kernel chooses per wave between one dark product per pixel and one per frame
(stack_fast_kernel, round 7), so the second must not cost more than it did.  One JSON line: ms per call of either form."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch
from astrophotography_amd import ops, synth
from bench_kernels import timeit

N, H, W = 64, 4096, 4096
masters = synth.make_masters(H, W, config_id=2, device='cuda')
nflat, _ = ops.flat_normalize(masters['flat'])
frames = synth.make_frames(N, masters, nflat, config_id=2)
uniform = torch.full((N,), synth.EXP_RATIO, dtype=torch.float32, device='cuda')
per_frame = uniform * (1.0 + 0.001 * torch.arange(N, dtype=torch.float32, device='cuda'))
res = {'kernel': ops.stack_kernel_name(N, 'f32', calibrated=True)}
for name, e in (('uniform', uniform), ('per_frame', per_frame)):
    calib = dict(bias=masters['bias'], dark=masters['dark'], nflat=nflat, exp_ratio=e)
    med, best = timeit(lambda: ops.stack_sigclip(frames, sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count')), reps=20, warm=5)
    res[name + '_ms'] = round(med, 4)
    res[name + '_min_ms'] = round(best, 4)
print(json.dumps(res))
