#!/usr/bin/env python3
"""tools/bench_input_grad.py -- k_grid_input_grad (nrc_grid_backward_input, 16 x 2, pair-major d_in) against k_grid_encode of the training query at the same
sample count, in one process: M = 264 000 (a training batch: 2 200 rays of the bench scene) and 8 Mi samples.

Both kernels read the same 8 corners x 16 levels per sample (512 B of table per sample: the HBM ruler); the encoder is the yardstick.  The samples are the
marched samples of rays of the bench scene (consecutive samples of a ray follow each other, as in a training batch).  k_grid_input_grad: HIP events around
LAUNCHES back-to-back launches; k_grid_encode: the library's own events behind the kernel (stage timer) over the same number of training-query forwards.
ROUNDS rounds, the two kernels alternating inside a round; median (fastest .. slowest round) per launch.

usage: bench_input_grad.py [--rounds 5] [--out profiles/r14_input_grad.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch

import bench
from nerficg_amd import _lib
from nerficg_amd.ngp import query_train
from nerficg_amd.raygen import generate_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r14_input_grad.json'))
args = ap.parse_args()

dev = torch.device('cuda', 0)
lib = _lib.load()
model, renderer, cam, poses = bench.build_scene(dev)
net = model.encoding_xyz
g = net.grid_cfg
cfg = (g['log2_hashmap_size'], g['base_resolution'], float(g['per_level_scale']))
mn, sz = renderer._box()


def marched_samples(m):
    """(m, 3) box-centred positions and directions of training samples: rays of the bench poses, marched with a seeded jitter"""
    n_rays = max(2200, m // 100)
    per_pose = -(-n_rays // 4)
    gen = torch.Generator().manual_seed(m)
    os_, ds_ = [], []
    for p in poses[:4]:
        rays = generate_rays(cam.width, cam.height, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, p, device=dev, want_direction=False)
        ids = torch.randperm(rays['origin'].shape[0], generator=gen)[:per_pose].to(dev)
        os_.append(rays['origin'][ids]); ds_.append(rays['view_direction'][ids])
    o, d, span = renderer.clip_rays(torch.cat(os_), torch.cat(ds_), cam)
    _, xyzs, dirs, *_ = renderer._march(o, d, span, 0.0, torch.rand(o.shape[0], generator=gen).to(dev))
    reps = -(-m // max(int(xyzs.shape[0]), 1))
    return xyzs.repeat(reps, 1)[:m].contiguous(), dirs.repeat(reps, 1)[:m].contiguous(), int(xyzs.shape[0])


def time_input_grad(x01, d_in, out, launches):
    m = x01.shape[0]
    table = net._table16()
    call = lambda: _lib.check(lib.nrc_grid_backward_input(_lib.ptr(x01), m, _lib.ptr(d_in), 1, _lib.ptr(table), g['n_levels'], 2, *cfg, _lib.ptr(out),
                                                          _lib.stream_of(out)), 'grid_backward_input')
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches * 1e3   # us


def time_encode(xyzs, dirs, launches):
    with _lib.stage_timer() as st:
        for _ in range(launches):
            query_train(net, model.color_mlp_with_encoding, xyzs, dirs, mn, sz)
        torch.cuda.synchronize()
    tot, _ = st.by_name()['k_grid_encode<train>']   # (all launches of the encoder inside one forward count as that forward's)
    return tot / launches * 1e3   # us


results = {'_meta': {'command': 'python tools/bench_input_grad.py --rounds %d' % args.rounds, 'grid': '16 x 2, T = 2^%d' % g['log2_hashmap_size'],
                     'table_bytes_per_sample': 512, 'hbm_peak_gbs': bench.HBM_PEAK_GBS, 'csrc_sha': bench.csrc_digests()}}
for label, m, launches in (('264K', 264_000, 50), ('8Mi', 8 << 20, 10)):
    xyzs, dirs, marched = marched_samples(m)
    x01 = ((xyzs - model.xyz_min) / model.xyz_size).contiguous()
    d_in = (torch.randn(16, m, 2, device=dev) * 1e-3).contiguous()
    out = torch.empty(m, 3, device=dev)
    net._half_params()
    with torch.enable_grad():
        for _ in range(3):   # warm-up of both
            time_input_grad(x01, d_in, out, 2)
            time_encode(xyzs, dirs, 2)
        rounds = []
        for r in range(args.rounds):
            rounds.append({'k_grid_input_grad_us': round(time_input_grad(x01, d_in, out, launches), 2), 'k_grid_encode_us': round(time_encode(xyzs, dirs, launches), 2)})
    ig = [r['k_grid_input_grad_us'] for r in rounds]
    en = [r['k_grid_encode_us'] for r in rounds]
    med_ig, med_en = statistics.median(ig), statistics.median(en)
    ruler_us = 512.0 * m / (bench.HBM_PEAK_GBS * 1e9) * 1e6
    results[label] = {'samples': m, 'marched_samples_tiled': marched, 'launches_per_round': launches, 'rounds': rounds,
                      'k_grid_input_grad_us': {'median': med_ig, 'min': min(ig), 'max': max(ig)},
                      'k_grid_encode_us': {'median': med_en, 'min': min(en), 'max': max(en)},
                      'ratio_input_grad_over_encode': round(med_ig / med_en, 3),
                      'hbm_ruler_us': round(ruler_us, 2), 'input_grad_fraction_of_hbm_ruler': round(ruler_us / med_ig, 4),
                      'encode_fraction_of_hbm_ruler': round(ruler_us / med_en, 4)}
    print(f'{label}: k_grid_input_grad {med_ig:.1f} us ({min(ig):.1f} .. {max(ig):.1f}), k_grid_encode<train> {med_en:.1f} us ({min(en):.1f} .. {max(en):.1f}), '
          f'ratio {med_ig / med_en:.3f}, 512 B/sample HBM ruler {ruler_us:.1f} us = {ruler_us / med_ig:.3f} of the kernel', flush=True)
    del xyzs, dirs, x01, d_in, out
    torch.cuda.empty_cache()
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(results, indent=1, sort_keys=True))
print('wrote', args.out)
