#!/usr/bin/env python3
"""tools/bench_nerf_fused.py -- the fused NeRF block (csrc/nerf_net.hip, nerf.fused_forward) against the torch module it replaces at inference,
in one process on one GPU, after warm-up, HIP events around every repeat:
  * the reference's chunk, 8192 rays x 256 samples (fine pass) and x 64 samples (coarse pass): fused kernel (one direction row per ray), NeRFBlock
    under no_grad in f32 (the reference's path), NeRFBlock.half() (for information);
  * one whole render_rays image at 200 x 200 (64 coarse + 192 fine samples), fused and torch.
Per entry: median, min and max of the repeats, TFLOP/s on 2 x MAC-per-sample (593 408 for the default block), the fraction of the 2.5 PFLOP/s fp16 MFMA
peak.  GATE (exit status 1 when missed): the fused median is below the f32 torch median at both chunk shapes.
Usage: python tools/bench_nerf_fused.py [repeats] [out.json]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from nerficg_amd import nerf
from tests import scenes

PEAK_FP16 = 2.5e15
repeats = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
assert torch.cuda.is_available(), 'bench_nerf_fused.py measures on the GPU'
dev = torch.device('cuda:0')
torch.manual_seed(0)
coarse, fine = nerf.NeRFBlock().to(dev), nerf.NeRFBlock().to(dev)
fine_half = nerf.NeRFBlock().to(dev)
fine_half.load_state_dict(fine.state_dict())
fine_half = fine_half.half()
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


def entry(ms, samples):
    med = float(np.median(ms))
    tf = 2.0 * mac * samples / (med * 1e-3) / 1e12
    return dict(median_ms=med, min_ms=float(min(ms)), max_ms=float(max(ms)), repeats=len(ms), tflops=tf, fraction_of_fp16_peak=tf * 1e12 / PEAK_FP16)


result = dict(device=torch.cuda.get_device_name(0), mac_per_sample=mac, flop_per_sample=2 * mac, peak_fp16_flops=PEAK_FP16, chunks={}, image={})
gate = True
with torch.no_grad():
    for label, n_samples in (('fine_8192x256', 256), ('coarse_8192x64', 64)):
        n_rays = 8192
        g = torch.Generator(device='cpu').manual_seed(1)
        pos = (torch.rand(n_rays * n_samples, 3, generator=g) * 8 - 4).to(dev)
        vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1).to(dev)
        expanded = vd[:, None, :].expand(-1, n_samples, -1).reshape(-1, 3)
        expanded_h, pos_h = expanded.half(), pos.half()
        m = pos.shape[0]
        e = dict(fused=entry(timed(lambda: nerf.fused_forward(fine, pos, vd, n_samples), repeats), m),
                 torch_f32=entry(timed(lambda: fine(pos, expanded), repeats), m),
                 torch_f16=entry(timed(lambda: fine_half(pos_h, expanded_h), repeats), m))
        e['speedup_vs_f32'] = e['torch_f32']['median_ms'] / e['fused']['median_ms']
        s_f, c_f = nerf.fused_forward(fine, pos[:65536], vd[:65536 // n_samples], n_samples)
        s_t, c_t = fine(pos[:65536], expanded[:65536])
        e['max_abs_diff_vs_f32'] = dict(sigma=float((s_f - s_t).abs().max()), rgb=float((c_f - c_t).abs().max()))
        gate = gate and e['fused']['median_ms'] < e['torch_f32']['median_ms']
        result['chunks'][label] = e
        print(label, json.dumps(e), flush=True)

    W = H = 200
    fx, fy, cx, cy = scenes.lego_intrinsics(W, H)
    c2w = np.eye(4); c2w[2, 3] = -4.0
    o, d, vdir = (torch.from_numpy(a).to(dev) for a in scenes.numpy_rays(W, H, c2w, fx, fy, cx, cy))
    bg = torch.ones(3, device=dev)
    image = lambda fused: nerf.render_rays(coarse, fine, o, d, vdir, 2.0, 6.0, bg, ray_batch_size=8192, n_samples_coarse_nerf=64, n_samples_nerf=192, fused=fused)
    n_net = W * H * (64 + 256)
    for label, fused in (('fused', True), ('torch_f32', False)):
        result['image'][label] = entry(timed(lambda: image(fused), repeats), n_net)
        result['image'][label]['krays_per_s'] = W * H / result['image'][label]['median_ms']
    a, b = image(True), image(False)
    result['image']['max_abs_rgb_diff'] = float((a['rgb'] - b['rgb']).abs().max())
    print('image_200x200', json.dumps(result['image']), flush=True)
result['gate_fused_below_torch_f32'] = bool(gate)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(result, indent=1) + '\n')
print('GATE', 'ok' if gate else 'MISSED')
sys.exit(0 if gate else 1)
