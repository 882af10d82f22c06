#!/usr/bin/env python3
"""tools/bench_gs_features.py [repeats=9] [out.json] -- the 3DGS feature pass against the only way to the same maps without it.

Scene: the bench's 1 M synthetic Gaussians at 1297x840 (bench.build_gs_scene).  For C = 3, 16, 32 and 64 channels, in ONE process, alternating per repeat:

  features   one rasterizer call with features=(P, C): colour + feature map, and with the backward: every gradient of <g_rgb, image> + <g_f, feature_map>
  emulation  the same colour call WITHOUT features plus ceil(C / 3) further rasterizer calls with colors_precomp triples and bg = 0 (tests/gs_depth_alpha_ref.py's
             trick: each repeats preprocess, sort, binning and the alpha evaluation), and with the backward one backward pass per call

Both sides therefore contain the plain colour frame; the time ADDED by the feature maps is the side's time minus the plain frame's, also measured here.  HIP events
around each side, median of `repeats` (>= 9) and the spread (min .. max) of each side, as the project's measuring practice asks: a difference counts only
when it exceeds the two spreads together.  Also: the time a plain training step (forward + backward of the colour frame) gains at C = 16, and the new kernels'
own durations from the library's stage timer.  Prints one JSON object; writes it to out.json when given."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import bench
from nerficg_amd import _lib
from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

REPEATS = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else None
CHANNELS = (3, 16, 32, 64)
dev = torch.device('cuda', 0)
gs = bench.build_gs_scene(dev)
t, rast, P, W, H = gs['tensors'], gs['rast'], gs['n'], gs['w'], gs['h']
rs0 = rast.raster_settings
rast_bg0 = GaussianRasterizer(rs0._replace(bg=torch.zeros(3, device=dev)))
gen = torch.Generator(device=dev).manual_seed(0)
g_rgb = torch.rand(3, H, W, device=dev, generator=gen)


def leaves(grad):
    a = {k: v.detach().requires_grad_(grad) for k, v in t.items()}
    a['means2D'] = torch.zeros_like(a['means3D'], requires_grad=grad)
    return a


def colour_call(a, **kw):
    return rast(means3D=a['means3D'], means2D=a['means2D'], opacities=a['opacities'], shs=a['shs'], scales=a['scales'], rotations=a['rotations'], **kw)


def plain(grad):
    a = leaves(grad)
    out = colour_call(a)
    if grad:
        out[0].backward(g_rgb)


def with_features(feats, g_f, grad):
    a = leaves(grad)
    f = feats.detach().requires_grad_(grad)
    out = colour_call(a, features=f)
    if grad:
        torch.autograd.backward([out[0], out[2]], [g_rgb, g_f])


def emulation(feats, g_f, grad):
    """The colour call, then one call per zero-padded triple of channels; the gradients of the calls accumulate in the same leaves."""
    a = leaves(grad)
    out = colour_call(a)
    if grad:
        out[0].backward(g_rgb)
    C = feats.shape[1]
    for k in range(0, C, 3):
        tri = torch.zeros(P, 3, device=dev)
        n = min(3, C - k)
        tri[:, :n] = feats[:, k:k + n]
        tri.requires_grad_(grad)
        img, _ = rast_bg0(means3D=a['means3D'], means2D=a['means2D'], opacities=a['opacities'], colors_precomp=tri, scales=a['scales'], rotations=a['rotations'])
        if grad:
            g3 = torch.zeros(3, H, W, device=dev)
            g3[:n] = g_f[k:k + n]
            img.backward(g3)


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


result = {'scene': f'{P} Gaussians, {W}x{H}', 'repeats': REPEATS, 'channels': {}}
for C in CHANNELS:
    feats = torch.randn(P, C, device=dev, generator=gen)
    g_f = torch.rand(C, H, W, device=dev, generator=gen)
    entry = {}
    for label, grad in (('forward', False), ('forward_backward', True)):
        r = timed({'plain': lambda: plain(grad), 'features': lambda: with_features(feats, g_f, grad), 'emulation': lambda: emulation(feats, g_f, grad)})
        added_f = r['features']['median_ms'] - r['plain']['median_ms']
        added_e = r['emulation']['median_ms'] - r['plain']['median_ms']
        spreads = (r['features']['max_ms'] - r['features']['min_ms']) + (r['emulation']['max_ms'] - r['emulation']['min_ms'])
        r.update(added_by_features_ms=round(added_f, 4), added_by_emulation_ms=round(added_e, 4), two_spreads_ms=round(spreads, 4),
                 features_beat_emulation_by_more_than_the_spreads=bool(r['emulation']['median_ms'] - r['features']['median_ms'] > spreads))
        entry[label] = r
    with _lib.stage_timer() as st:
        for _ in range(3):
            with_features(feats, g_f, True)
    entry['stage_ms'] = {k: round(tot / 3, 4) for k, (tot, cnt) in st.by_name().items() if 'features' in k or k in ('k_render', 'k_render_bw', 'zero')}
    result['channels'][str(C)] = entry
    if C == 16:
        result['training_step_gain_at_C16_ms'] = entry['forward_backward']['added_by_features_ms']
print(json.dumps(result))
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(result, indent=1))
