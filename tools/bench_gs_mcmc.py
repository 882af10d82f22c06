#!/usr/bin/env python3
"""tools/bench_gs_mcmc.py [repeats] [out.json] -- the 3DGS-MCMC steps at 1 M and 6 M Gaussians (include/nerficg_hip.h group 16), HIP events, 5 warm-up rounds, medians
and minima over `repeats` (default 30, at least 20):

  * the SGLD noise: nerficg_amd.gaussian_splatting.mcmc_noise with the kernel's own generator, and with the caller's draw, against the published tensor
    expression (tests/gs_mcmc_ref.noise_torch, f32 on the same GPU) without and with its torch.randn; kernel and expression interleaved in one process;
  * the kernel's share of its byte model: 56 B per Gaussian (16 rotation + 12 log-scale + 4 logit + 12 position read, 12 written) at 8 TB/s;
  * one relocation round (Gaussians.relocate) with 5 % dead rows: the whole call, host logic and its two host reads included, and the relocation launch alone;
  * the regulariser (two launches).

One JSON line on stdout, and in the file named by the second argument when there is one."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch

from nerficg_amd.gaussian_splatting import Gaussians, _mcmc_relocation, mcmc_noise, mcmc_regulariser_grads
from tests.gs_mcmc_ref import noise_torch

repeats = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 30)
WARM = 5
dev = torch.device('cuda', 0)
LR, NOISE_LR = 0.00016, 5e5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def summary(ts):
    return {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'repeats': len(ts)}


result = {}
for P in (1_000_000, 6_000_000):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(P, 3, device=dev, generator=gen) * 4 - 2
    rot = torch.randn(P, 4, device=dev, generator=gen)
    log_scales = torch.log(0.003 + 0.05 * torch.rand(P, 3, device=dev, generator=gen))
    opacity = torch.rand(P, 1, device=dev, generator=gen) * 0.3 * (torch.rand(P, 1, device=dev, generator=gen) < 0.3) + 0.002
    logits = torch.log(opacity / (1 - opacity))
    z = torch.randn(P, 3, device=dev, generator=gen)
    sink = [None]
    it = [0]

    def kernel_generator():
        it[0] += 1
        mcmc_noise(x, rot, log_scales, logits, LR, noise_lr=NOISE_LR, seed=1, iteration=it[0])

    def kernel_z():
        mcmc_noise(x, rot, log_scales, logits, LR, noise_lr=NOISE_LR, z=z)

    def tensor_z():
        sink[0] = noise_torch(x, rot, log_scales, logits, z, LR, NOISE_LR)

    def tensor_randn():
        sink[0] = noise_torch(x, rot, log_scales, logits, torch.randn_like(x), LR, NOISE_LR)

    paths = {'kernel_generator': kernel_generator, 'kernel_z_in': kernel_z, 'tensor_expression_z_given': tensor_z, 'tensor_expression_with_randn': tensor_randn}
    times = {k: [] for k in paths}
    for r in range(repeats + WARM):
        for k, f in paths.items():
            t = timed(f)
            if r >= WARM:
                times[k].append(t)
    entry = {k: summary(v) for k, v in times.items()}
    model_us = 56.0 * P / 8e12 * 1e6
    entry['byte_model'] = {'bytes_per_gaussian': 56, 'at_8TBps_us': round(model_us, 2),
                           'fraction_kernel_z_in': round(model_us / statistics.median(times['kernel_z_in']), 3),
                           'fraction_kernel_generator': round(model_us / statistics.median(times['kernel_generator']), 3)}
    entry['speedup_vs_tensor_expression_with_randn'] = round(statistics.median(times['tensor_expression_with_randn']) / statistics.median(times['kernel_generator']), 1)
    sink[0] = None

    # regulariser
    g_o, g_s = torch.zeros(P, 1, device=dev), torch.zeros(P, 3, device=dev)
    ts = [timed(lambda: mcmc_regulariser_grads(logits, log_scales, g_o, g_s)) for _ in range(repeats + WARM)][WARM:]
    entry['regulariser'] = summary(ts)
    del g_o, g_s

    # one relocation round, 5 % dead rows
    g = Gaussians(x.clone(), log_scales.clone(), rot.clone(), logits.clone(), torch.zeros(P, 1, 3, device=dev), torch.zeros(P, 15, 3, device=dev))
    g.training_setup()
    for p in g._six():
        p.grad = torch.zeros_like(p)
    g.optimizer.step()                                      # creates both moments of the six groups
    dead_rows = torch.randperm(P, device=dev, generator=gen)[:P // 20]
    alive_logits = g._opacities.data.clone().clamp_min(-3.0)
    whole, launch = [], []
    for r in range(repeats + WARM):
        g._opacities.data.copy_(alive_logits)
        g._opacities.data[dead_rows] = -9.0                 # o = 1.2e-4: dead
        t = timed(lambda: sink.__setitem__(0, g.relocate()))
        counts = torch.bincount(torch.randint(0, P, (P // 20,), device=dev, generator=gen), minlength=P).to(torch.int32)
        t2 = timed(lambda: _mcmc_relocation(g._opacities.data, g._scales.data, counts, g._adam_moments()))
        if r >= WARM:
            whole.append(t)
            launch.append(t2)
    assert sink[0]['n_dead'] == P // 20 == sink[0]['n_relocated']
    entry['relocation_round_5pct_dead'] = summary(whole)
    entry['relocation_launch_5pct_drawn'] = summary(launch)
    result[f'P={P}'] = entry
    del g, x, rot, log_scales, logits, z
    torch.cuda.empty_cache()

line = json.dumps({'tool': 'bench_gs_mcmc', 'device': torch.cuda.get_device_name(0), 'results': result})
print(line)
if len(sys.argv) > 2:
    Path(sys.argv[2]).write_text(line + '\n')
