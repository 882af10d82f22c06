#!/usr/bin/env python3
"""tools/bench_nerf_input_grad.py -- a pose-refinement iteration of the vanilla NeRF path at the yaml sizes (1024 rays, 64 coarse samples, the fine pass
on 64 + 192 = 256 samples per ray: 65 536 and 262 144 block rows), in one process on one GPU, after warm-up, HIP events around every repeat, medians:
  * the iteration -- render_rays(fused_train=True, device_rays=True) from ray origins, directions and viewing directions that require grad, against the
    FROZEN blocks -> MSE on both passes -> backward -> Adam.step on the three ray tensors -- through the fused path with input_grad=True (header group 20);
  * the same call without the flag: the behaviour before group 20, where a ray tensor that requires grad sends every stage to its torch fallback;
  * the new launches alone (k_nerf_input_grad, k_nerf_dir_reduce, k_nerf_positions_bw, k_nerf_integrate_bw_dirs), per pass, from the library's stage
    timer, and the byte model of the block kernel: it reads G[H_1], G[H_6] and G[C_1], (256 + 256 + 128) fp16 = 1280 bytes per row, and writes 24.
Every number under "measured" is a median; everything under "derived" is arithmetic on those.  No gate.
Usage: python tools/bench_nerf_input_grad.py [repeats] [out.json]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from nerficg_amd import _lib, nerf

repeats = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else None
assert torch.cuda.is_available(), 'bench_nerf_input_grad.py measures on the GPU'
dev = torch.device('cuda:0')
torch.manual_seed(0)
coarse, fine = nerf.NeRFBlock().to(dev), nerf.NeRFBlock().to(dev)
with torch.no_grad():
    for b in (coarse, fine):
        b.density_layer.bias.fill_(0.5)
        for p in b.parameters():
            p.requires_grad_(False)
NEAR, FAR, SC, SF, N = 2.0, 6.0, 64, 192, 1024
STREAM_BYTES_PER_S = 6.3e12      # the achievable HBM streaming rate the byte model is held against
NEW = ('k_nerf_input_grad', 'k_nerf_dir_reduce', 'k_nerf_positions_bw', 'k_nerf_integrate_bw_dirs')


def timed(fn, n=repeats):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), repeats=len(ms))


g = torch.Generator(device='cpu').manual_seed(2)
o = (torch.randn(N, 3, generator=g) * 0.3).to(dev).requires_grad_()
d = torch.randn(N, 3, generator=g).to(dev).requires_grad_()
vd = torch.nn.functional.normalize(d.detach(), dim=-1).requires_grad_()
target = torch.rand(N, 3, generator=g).to(dev)
bg = torch.ones(3, device=dev)
opt = torch.optim.Adam([o, d, vd], lr=1e-4)


def iteration(flag):
    opt.zero_grad(set_to_none=True)
    out = nerf.render_rays(coarse, fine, o, d, vd, NEAR, FAR, bg, n_samples_coarse_nerf=SC, n_samples_nerf=SF, randomize_samples=True, fused_train=True,
                           device_rays=True, input_grad=flag)
    ((out['rgb'] - target).square().mean() + (out['rgb_coarse'] - target).square().mean()).backward()
    opt.step()


def stage_ms(fn, n=repeats):
    """per kernel name: the medians of the library's own stage timer, one list entry per launch of that name inside fn (coarse pass first in the forward,
    last in the backward)"""
    per = {}
    for _ in range(n):
        with _lib.stage_timer() as timer:
            fn()
        count = {}
        for name, ms in timer.stages:
            k = count.get(name, 0)
            count[name] = k + 1
            per.setdefault((name, k), []).append(ms)
    out = {}
    for (name, k), v in sorted(per.items()):
        out.setdefault(name, []).append(float(np.median(v)))
    return out


result = dict(device=torch.cuda.get_device_name(0), rays=N, samples=[SC, SF], block_rows=[N * SC, N * (SC + SF)], repeats=repeats, measured={}, derived={})
result['measured']['iteration_input_grad'] = timed(lambda: iteration(True))
result['measured']['iteration_torch_fallback'] = timed(lambda: iteration(False))
stages = stage_ms(lambda: iteration(True))
result['measured']['stage_timer_ms'] = stages
fallback_stages = stage_ms(lambda: iteration(False), n=3)
result['measured']['fallback_launches_of_the_library'] = sorted(fallback_stages)
it_new, it_old = result['measured']['iteration_input_grad']['median_ms'], result['measured']['iteration_torch_fallback']['median_ms']
new_ms = sum(sum(stages.get(k, [])) for k in NEW)
backward_ms = sum(sum(stages.get(k, [])) for k in ('k_nerf_head_max', 'k_nerf_dgrad', 'k_nerf_wgrad', 'k_nerf_wreduce'))
rows_fine = N * (SC + SF)
kernel_fine_ms = max(stages.get('k_nerf_input_grad', [0.0]))       # the 262 144-row launch is the longer of the two
model_bytes = rows_fine * (1280 + 24)
result['derived'] = dict(speedup_over_the_fallback=it_old / it_new, new_launches_ms=new_ms, block_backward_launches_ms=backward_ms,
                         new_launches_over_block_backward=new_ms / backward_ms if backward_ms else None,
                         input_grad_kernel_fine_pass_ms=kernel_fine_ms, byte_model_bytes=model_bytes,
                         byte_model_ms=model_bytes / STREAM_BYTES_PER_S * 1e3,
                         achieved_gbytes_per_s=model_bytes / (kernel_fine_ms * 1e-3) / 1e9 if kernel_fine_ms else None,
                         fraction_of_byte_model=(model_bytes / STREAM_BYTES_PER_S * 1e3) / kernel_fine_ms if kernel_fine_ms else None)
print(json.dumps(result), flush=True)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(result, indent=1) + '\n')
