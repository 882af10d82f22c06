#!/usr/bin/env python3
"""tools/bench_nerf_rays.py -- the NeRF ray stages (csrc/nerf_rays.hip: nerf.sample_coarse / composite / sample_fine, render_rays(device_rays=True))
against the torch expressions they replace, in one process on one GPU, after warm-up, HIP events around every repeat, medians:
  * the training iteration at 1024 rays, 64 + 192 samples (render_rays(randomize_samples=True, fused_train=True) -> MSE -> backward -> Adam.step) as it
    is WITHOUT device_rays, and its parts measured on their own: the two blocks (forward + backward), sampling + sort, compositing forward + backward,
    MSE + Adam -- so that "everything outside the blocks" is a measurement, not a subtraction;
  * the same iteration and the same parts with device_rays=True;
  * the stages alone at 1024 x 64 and 1024 x 256 (resampling: 1024 x (64 -> 192)), device against torch, with the achieved bytes per second on the
    stage's compulsory traffic (every input read once, every output written once) and the library's stage timer for the kernel itself;
  * one 8192-ray inference chunk (render_rays under no_grad, fused=True) with and without device_rays.
Every number under "measured" is a median of HIP-event intervals; everything under "derived" is arithmetic on those.  No gate.
Usage: python tools/bench_nerf_rays.py [repeats] [out.json]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from nerficg_amd import _lib, nerf

repeats = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else None
assert torch.cuda.is_available(), 'bench_nerf_rays.py measures on the GPU'
dev = torch.device('cuda:0')
torch.manual_seed(0)
coarse, fine = nerf.NeRFBlock().to(dev), nerf.NeRFBlock().to(dev)
with torch.no_grad():
    for b in (coarse, fine):
        b.density_layer.bias.fill_(0.5)
NEAR, FAR, SC, SF = 2.0, 6.0, 64, 192


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


def kernel_ms(fn, n=repeats):
    """per kernel name: the median of the library's own stage timer (events directly around the launch)"""
    per = {}
    for _ in range(n):
        with _lib.stage_timer() as timer:
            fn()
        for name, ms in timer.stages:
            per.setdefault(name, []).append(ms)
    return {k: float(np.median(v)) for k, v in per.items() if k.startswith('k_nerf_sample') or k.startswith('k_nerf_integrate')}


def rays(n, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    o = (torch.randn(n, 3, generator=g) * 0.3).to(dev)
    d = torch.randn(n, 3, generator=g).to(dev)
    return o, d, torch.nn.functional.normalize(d, dim=-1), torch.rand(n, 3, generator=g).to(dev)


n_rays = 1024
o, d, vdir, target = rays(n_rays, 2)
bg = torch.ones(3, device=dev)
opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)


def iteration(device_rays):
    opt.zero_grad(set_to_none=True)
    out = nerf.render_rays(coarse, fine, o, d, vdir, NEAR, FAR, bg, n_samples_coarse_nerf=SC, n_samples_nerf=SF, randomize_samples=True, fused_train=True,
                           device_rays=device_rays)
    ((out['rgb'] - target).square().mean() + (out['rgb_coarse'] - target).square().mean()).backward()
    opt.step()


def torch_positions(t):
    return (o[:, None, :] + d[:, None, :] * t[:, :, None]).reshape(-1, 3)


def make_parts(device_rays):
    """the pieces of one iteration as closures over fixed inputs of the right shapes"""
    t_c = nerf.generate_samples(n_rays, SC, NEAR, FAR, True, torch.float32, dev)
    g = torch.Generator(device='cpu').manual_seed(5)
    w_c = (torch.rand(n_rays, SC, generator=g) ** 8).to(dev)
    t_all = torch.sort(torch.cat((t_c, nerf.generate_samples_from_pdf(t_c, w_c, SF, True)), dim=-1), dim=-1).values
    pos = {SC: torch_positions(t_c).contiguous(), SC + SF: torch_positions(t_all).contiguous()}
    ts = {SC: t_c.contiguous(), SC + SF: t_all.contiguous()}
    sig = {s: (torch.rand(n_rays, s, generator=g) * 3).to(dev).requires_grad_() for s in ts}
    col = {s: torch.rand(n_rays, s, 3, generator=g).to(dev).requires_grad_() for s in ts}
    out_rgb = torch.rand(n_rays, 3, generator=g).to(dev).requires_grad_()
    out_rgb_c = torch.rand(n_rays, 3, generator=g).to(dev).requires_grad_()

    def blocks():
        for blk, s in ((coarse, SC), (fine, SC + SF)):
            blk.zero_grad(set_to_none=True)
            sigma, rgb = nerf.fused_apply(blk, pos[s], vdir, s)
            (sigma.sum() * 1e-3 + rgb.sum() * 1e-3).backward()

    def sampling():
        if device_rays:
            t, _ = nerf.sample_coarse(o, d, SC, NEAR, FAR, True)
            nerf.sample_fine(t, w_c, SF, True, o, d)
        else:
            t = nerf.generate_samples(n_rays, SC, NEAR, FAR, True, torch.float32, dev)
            torch_positions(t)
            t2, _ = torch.sort(torch.cat((t, nerf.generate_samples_from_pdf(t, w_c, SF, True)), dim=-1), dim=-1)
            torch_positions(t2)

    def compositing():
        for s in ts:
            sig[s].grad = col[s].grad = None
            rgb, _, alpha, w = (nerf.composite if device_rays else nerf.integrate_samples)(ts[s], d, sig[s], col[s], bg)
            (rgb - target).square().mean().backward()

    def mse_adam():
        out_rgb.grad = out_rgb_c.grad = None
        ((out_rgb - target).square().mean() + (out_rgb_c - target).square().mean()).backward()
        opt.step()                                   # the parameters keep the gradients of the last whole iteration
    return dict(blocks=blocks, sampling_and_sort=sampling, compositing_fw_bw=compositing, mse_and_adam=mse_adam)


result = dict(device=torch.cuda.get_device_name(0), rays=n_rays, samples=[SC, SF], repeats=repeats, measured={}, derived={})
for label, flag in (('torch_rays', False), ('device_rays', True)):
    m = dict(iteration=timed(lambda: iteration(flag)))
    for name, fn in make_parts(flag).items():
        m[name] = timed(fn)
    result['measured'][label] = m
    parts = sum(m[k]['median_ms'] for k in ('blocks', 'sampling_and_sort', 'compositing_fw_bw', 'mse_and_adam'))
    result['derived'][label] = dict(sum_of_parts_ms=parts, iteration_minus_blocks_ms=m['iteration']['median_ms'] - m['blocks']['median_ms'],
                                    iteration_minus_sum_of_parts_ms=m['iteration']['median_ms'] - parts)
    print(label, json.dumps(m), json.dumps(result['derived'][label]), flush=True)
result['derived']['iteration_speedup'] = (result['measured']['torch_rays']['iteration']['median_ms'] /
                                          result['measured']['device_rays']['iteration']['median_ms'])

# ---- the stages alone, device against torch, on their compulsory traffic
stages = {}
g = torch.Generator(device='cpu').manual_seed(7)
for s in (64, 256):
    u = torch.rand(n_rays, s, generator=g).to(dev)
    t = nerf.sample_coarse(o, d, s, NEAR, FAR, True, u=u)[0]
    sigma = (torch.rand(n_rays, s, generator=g) * 3).to(dev)
    rgb = torch.rand(n_rays, s, 3, generator=g).to(dev)
    t_row = torch.linspace(NEAR, FAR, s, device=dev).expand(n_rays, s)
    up = [torch.randn(n_rays, 3, generator=g).to(dev), torch.randn(n_rays, 1, generator=g).to(dev), torch.randn(n_rays, s, generator=g).to(dev)]

    def torch_bw(leaf_s, leaf_c):
        leaf_s.grad = leaf_c.grad = None
        r, _, a, w = nerf.integrate_samples(t, d, leaf_s, leaf_c, bg)
        ((up[0] * r).sum() + (up[1] * a).sum() + (up[2] * w).sum()).backward()

    def device_bw(leaf_s, leaf_c):
        leaf_s.grad = leaf_c.grad = None
        r, _, a, w = nerf.composite(t, d, leaf_s, leaf_c, bg)
        ((up[0] * r).sum() + (up[1] * a).sum() + (up[2] * w).sum()).backward()
    ls, lc = sigma.clone().requires_grad_(), rgb.clone().requires_grad_()
    per = n_rays * s
    cases = {
        f'sample_coarse_{n_rays}x{s}': (lambda: nerf.sample_coarse(o, d, s, NEAR, FAR, True, u=u), lambda: torch_positions(nerf._stratified(t_row, u)),
                                        'k_nerf_sample_coarse', per * 20 + n_rays * 24),
        f'composite_forward_{n_rays}x{s}': (lambda: nerf.composite(t, d, sigma, rgb, bg), lambda: nerf.integrate_samples(t, d, sigma, rgb, bg),
                                            'k_nerf_integrate_fw', per * 24 + n_rays * 32),
        f'composite_forward_backward_{n_rays}x{s}': (lambda: device_bw(ls, lc), lambda: torch_bw(ls, lc), 'k_nerf_integrate_bw', per * 40 + n_rays * 28),
    }
    if s == 64:
        w = nerf.composite(t, d, sigma, rgb, bg)[3]
        uf = torch.rand(n_rays, SF, generator=g).to(dev)
        cases[f'sample_fine_{n_rays}x{SC}to{SF}'] = (
            lambda: nerf.sample_fine(t, w, SF, True, o, d, u=uf),
            lambda: torch_positions(torch.sort(torch.cat((t, nerf._samples_from_pdf(t, w, uf)), dim=-1), dim=-1).values),
            'k_nerf_sample_fine', n_rays * (SC * 8 + SF * 4 + 24 + (SC + SF) * 16))
    for name, (device_fn, torch_fn, kernel, traffic) in cases.items():
        e = dict(device=timed(device_fn), torch=timed(torch_fn), kernel_ms=kernel_ms(device_fn).get(kernel), compulsory_bytes=traffic)
        stages[name] = e
        result['derived'][name] = dict(speedup=e['torch']['median_ms'] / e['device']['median_ms'],
                                       call_gbytes_per_s=traffic / (e['device']['median_ms'] * 1e-3) / 1e9,
                                       kernel_gbytes_per_s=None if not e['kernel_ms'] else traffic / (e['kernel_ms'] * 1e-3) / 1e9)
        print(name, json.dumps(e), json.dumps(result['derived'][name]), flush=True)
result['measured']['stages'] = stages

# ---- one inference chunk
o8, d8, v8, _ = rays(8192, 3)


def chunk(flag):
    with torch.no_grad():
        nerf.render_rays(coarse, fine, o8, d8, v8, NEAR, FAR, bg, n_samples_coarse_nerf=SC, n_samples_nerf=SF, fused=True, device_rays=flag)


result['measured']['inference_chunk_8192'] = dict(torch_rays=timed(lambda: chunk(False)), device_rays=timed(lambda: chunk(True)))
c = result['measured']['inference_chunk_8192']
result['derived']['inference_chunk_8192_speedup'] = c['torch_rays']['median_ms'] / c['device_rays']['median_ms']
print('inference_chunk_8192', json.dumps(c), flush=True)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(result, indent=1) + '\n')
