#!/usr/bin/env python3
"""tools/bench_nerf_train.py -- the fused NeRF block's training path (csrc/nerf_net.hip k_nerf_forward<W, 2>, csrc/nerf_grad.hip, nerf.fused_apply) against
the torch paths it replaces, in one process on one GPU, after warm-up, HIP events around every repeat:
  * block forward + backward at the training shapes, 1024 rays x 64 samples (M = 65 536) and 1024 x 256 (M = 262 144): fused_apply (one direction row per
    ray), NeRFBlock under torch autograd in f32 (the reference's path), the same module under fp16 autocast; for the fused path also the library's
    stage timer per pass (training forward, scale + data gradient, weight gradient, reduction);
  * one whole training iteration at 1024 rays, 64 + 192 samples: render_rays(randomize_samples=True) -> MSE -> backward -> Adam.step, fused_train and torch.
Per entry: median, min and max of the repeats, TFLOP/s on 6 x MAC-per-sample (593 408 for the default block; per pass: 2 x), the fraction of the
2.5 PFLOP/s fp16 MFMA peak.  No gate: the numbers are reported as they come.
Usage: python tools/bench_nerf_train.py [repeats] [out.json]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from nerficg_amd import _lib, nerf

PEAK_FP16 = 2.5e15
repeats = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
assert torch.cuda.is_available(), 'bench_nerf_train.py measures on the GPU'
dev = torch.device('cuda:0')
torch.manual_seed(0)
coarse, fine = nerf.NeRFBlock().to(dev), nerf.NeRFBlock().to(dev)
with torch.no_grad():
    for b in (coarse, fine):
        b.density_layer.bias.fill_(0.5)     # an open density head: a closed one has no gradient to compute
mac = sum(lin.weight.numel() for lin in nerf._block_linears(fine))


def timed(fn, n):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def entry(ms, samples, flop_per_mac=6.0):
    med = float(np.median(ms))
    tf = flop_per_mac * mac * samples / (med * 1e-3) / 1e12
    return dict(median_ms=med, min_ms=float(min(ms)), max_ms=float(max(ms)), repeats=len(ms), tflops=tf, fraction_of_fp16_peak=tf * 1e12 / PEAK_FP16)


result = dict(device=torch.cuda.get_device_name(0), mac_per_sample=mac, flop_per_sample_forward_backward=6 * mac, peak_fp16_flops=PEAK_FP16, block={}, iteration={})
for label, n_samples in (('coarse_1024x64', 64), ('fine_1024x256', 256)):
    n_rays = 1024
    g = torch.Generator(device='cpu').manual_seed(1)
    pos = (torch.rand(n_rays * n_samples, 3, generator=g) * 8 - 4).to(dev)
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1).to(dev)
    expanded = vd[:, None, :].expand(-1, n_samples, -1).reshape(-1, 3).contiguous()
    m = pos.shape[0]
    w_s, w_c = (torch.randn(m, 1, generator=g) * 1e-3).to(dev), (torch.randn(m, 3, generator=g) * 1e-3).to(dev)

    def run(forward):
        fine.zero_grad(set_to_none=True)
        sigma, rgb = forward()
        ((sigma * w_s).sum() + (rgb * w_c).sum()).backward()

    def autocast():
        with torch.autocast('cuda', dtype=torch.float16):
            return fine(pos, expanded)
    e = dict(fused=entry(timed(lambda: run(lambda: nerf.fused_apply(fine, pos, vd, n_samples)), repeats), m),
             torch_f32=entry(timed(lambda: run(lambda: fine(pos, expanded)), repeats), m),
             torch_autocast_f16=entry(timed(lambda: run(autocast), repeats), m))
    passes = {}
    for _ in range(repeats):
        with _lib.stage_timer() as timer:
            run(lambda: nerf.fused_apply(fine, pos, vd, n_samples))
        for name, ms in timer.stages:
            passes.setdefault(name, []).append(ms)
    e['fused_passes'] = {name: entry(ms, m, 2.0) for name, ms in passes.items()}
    e['speedup_vs_f32'] = e['torch_f32']['median_ms'] / e['fused']['median_ms']
    e['speedup_vs_autocast_f16'] = e['torch_autocast_f16']['median_ms'] / e['fused']['median_ms']
    run(lambda: nerf.fused_apply(fine, pos, vd, n_samples))
    fused_grads = [p.grad.clone() for p in fine.parameters()]
    e['grad_stats'] = nerf.fused_grad_stats(fine).tolist()
    run(lambda: fine(pos, expanded))
    e['max_rel_grad_diff_vs_f32'] = max(float((a - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for a, p in zip(fused_grads, fine.parameters()))
    result['block'][label] = e
    print(label, json.dumps(e), flush=True)

n_rays = 1024
g = torch.Generator(device='cpu').manual_seed(2)
o = (torch.randn(n_rays, 3, generator=g) * 0.3).to(dev)
d = torch.randn(n_rays, 3, generator=g).to(dev)
vdir = torch.nn.functional.normalize(d, dim=-1)
target = torch.rand(n_rays, 3, generator=g).to(dev)
bg = torch.ones(3, device=dev)
opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)


def iteration(fused_train):
    opt.zero_grad(set_to_none=True)
    out = nerf.render_rays(coarse, fine, o, d, vdir, 2.0, 6.0, bg, n_samples_coarse_nerf=64, n_samples_nerf=192, randomize_samples=True, fused_train=fused_train)
    loss = (out['rgb'] - target).square().mean() + (out['rgb_coarse'] - target).square().mean()
    loss.backward()
    opt.step()


n_net = n_rays * (64 + 256)
for label, fused_train in (('fused_train', True), ('torch_f32', False)):
    result['iteration'][label] = entry(timed(lambda: iteration(fused_train), repeats), n_net)
    result['iteration'][label]['krays_per_s'] = n_rays / result['iteration'][label]['median_ms']
result['iteration']['speedup_vs_f32'] = result['iteration']['torch_f32']['median_ms'] / result['iteration']['fused_train']['median_ms']
print('iteration_1024', json.dumps(result['iteration']), flush=True)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(result, indent=1) + '\n')
