#!/usr/bin/env python3
"""tools/bench_gs_contributions.py [repeats=9] [out.json] -- the per-Gaussian contribution pass of the 3DGS rasterizer against the frame it scores and against the
only way to `weight_sum` without it.

Scene: the bench's 1 M synthetic Gaussians at 1297x840 (bench.build_gs_scene), a random non-negative pixel map with a quarter of exact zeros.  In ONE process,
alternating per repeat, each body between its own pair of HIP events:

  frame              the colour frame under no_grad (what an evaluation loop renders anyway)
  frame_and_stats    the same frame followed by rasterizer.contributions(m): all three statistics
  detour             features = ones(P, 1) through the feature pass, forward + backward with the map as the gradient of the (1, H, W) feature map:
                     features.grad is weight_sum -- and nothing gives weight_max or hits
  launch             contributions(m) alone on the kept state of one frame: with all three outputs, and with each output alone

Median of `repeats` (>= 9) and the spread (min .. max) of every body, as the project's measuring practice asks: a difference counts only when it exceeds the two
spreads together.  Also the kernel's own duration from the library's stage timer and the byte model of the launch (point_list + records + n_contrib + map + three
atomics per (tile, Gaussian) that has something to add), with the (tile, Gaussian) pairs counted from the result.  Prints one JSON object; writes it to out.json
when given."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import bench
from nerficg_amd import _lib

REPEATS = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device('cuda', 0)
gs = bench.build_gs_scene(dev)
t, rast, P, W, H = gs['tensors'], gs['rast'], gs['n'], gs['w'], gs['h']
gen = torch.Generator(device=dev).manual_seed(0)
m = torch.rand(H, W, device=dev, generator=gen) * (torch.rand(H, W, device=dev, generator=gen) >= 0.25)
ones = torch.ones(P, 1, device=dev)


def frame(**kw):
    a = {k: v.detach() for k, v in t.items()}
    return rast(means3D=a['means3D'], means2D=torch.zeros_like(a['means3D']), opacities=a['opacities'], shs=a['shs'], scales=a['scales'], rotations=a['rotations'], **kw)


def plain():
    with torch.no_grad():
        frame()


def with_stats():
    with torch.no_grad():
        frame()
    rast.contributions(m)


def detour():
    f = ones.detach().requires_grad_(True)
    out = frame(features=f)
    out[2].backward(m[None])
    return f.grad


def timed(bodies):
    """bodies: name -> callable.  One warm-up each, then REPEATS rounds in which every body runs once between its own pair of events (alternating sides)."""
    for b in bodies.values():
        b()
    torch.cuda.synchronize()
    ms = {k: [] for k in bodies}
    for _ in range(REPEATS):
        for k, b in bodies.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in ms.items()}


result = {'scene': f'{P} Gaussians, {W}x{H}', 'repeats': REPEATS}
r = timed({'frame': plain, 'frame_and_stats': with_stats, 'detour': detour})
spread = lambda k: r[k]['max_ms'] - r[k]['min_ms']
r['added_by_stats_ms'] = round(r['frame_and_stats']['median_ms'] - r['frame']['median_ms'], 4)
r['added_by_detour_ms'] = round(r['detour']['median_ms'] - r['frame']['median_ms'], 4)
r['two_spreads_ms'] = round(spread('frame_and_stats') + spread('detour'), 4)
r['stats_beat_detour_by_more_than_the_spreads'] = bool(r['detour']['median_ms'] - r['frame_and_stats']['median_ms'] > spread('frame_and_stats') + spread('detour'))
result['bodies'] = r

plain()                                   # the state the launches below run on
out = rast.contributions(m)
only = lambda key: (lambda: rast.contributions(m, out=out, clear=True, **{k: k == key for k in ('weight_sum', 'weight_max', 'hits')}))
result['launch'] = timed({'all_three': lambda: rast.contributions(m, out=out, clear=True), 'weight_sum_only': only('weight_sum'), 'weight_max_only': only('weight_max'),
                          'hits_only': only('hits'), 'all_three_no_map': lambda: rast.contributions(None, out=out, clear=True)})
with _lib.stage_timer() as st:
    for _ in range(5):
        rast.contributions(m, out=out, clear=True)
result['stage_ms'] = {k: round(tot / 5, 4) for k, (tot, cnt) in st.by_name().items()}

# the detour and the pass agree (both f32 sums of the same non-negative addends)
got, want = rast.contributions(m, out=out, clear=True)['weight_sum'], detour()[:, 0]
result['largest_relative_difference_to_the_detour'] = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
# byte model: what the launch must move at least
state = rast._frame_state
n_inst = int(state['point_list'].numel())
hit = out['hits'] > 0
result['counts'] = {'instances': n_inst, 'gaussians_hit': int(hit.sum()), 'hits': int(out['hits'].sum().item())}
# (tile, Gaussian) pairs with something to add are at most the instances; the model takes the instances as the upper bound and the hit Gaussians as the lower
model = lambda pairs: 4 * n_inst + 64 * n_inst + 4 * H * W + 4 * H * W + 3 * 4 * pairs
result['byte_model'] = {'upper_bytes': model(n_inst), 'lower_bytes': model(int(hit.sum())),
                        'terms': 'point_list 4 B + record 64 B per instance, n_contrib and the map 4 B per pixel each, three 4-byte atomics per (tile, Gaussian) pair'}
k_ms = result['stage_ms'].get('k_gs_contributions')
if k_ms:
    result['byte_model']['upper_GBps_at_kernel_time'] = round(model(n_inst) / (k_ms * 1e-3) / 1e9, 1)
print(json.dumps(result))
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(result, indent=1))
