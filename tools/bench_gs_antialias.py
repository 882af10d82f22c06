#!/usr/bin/env python3
"""tools/bench_gs_antialias.py [rounds=7] [out.json] [--parent DIR] | --body [antialiasing] -- what antialiasing=True costs, and that the default path is the parent's.

Scene: the bench's 1 M synthetic Gaussians at 1297x840 (bench.build_gs_scene), as tools/bench_gs_absgrad.py.  Three measurements, all in ONE call:
  1. k_preprocess and k_preprocess_bw with and without the flag: the library's stage timer (HIP events behind each launch, _lib.stage_timer) over 10 training
     frames per round, the two sides alternating per round in one process; median and spread (min .. max) over the rounds.
  2. The default path of this tree against the parent commit's (`--parent DIR`: a checkout of the parent with its library built): the same two kernels and the
     whole forward + backward, measured by `--body` child processes ALTERNATING between the two trees, `rounds` processes each.  The bar: this tree's medians lie
     inside the parent's own spread on the same lease.  Without --parent the leg is skipped and the JSON says so.
  3. nrc_gs_filter3d at 1 M Gaussians x 200 views against the torch loop of the published function (float32 on the device), HIP events, median of `rounds`.
No speed is promised.  Prints one JSON object; writes it to out.json when given (profiles/r32_gs_antialias.json)."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
argv = sys.argv[1:]
BODY = '--body' in argv
PARENT = str(Path(argv[argv.index('--parent') + 1]).resolve()) if '--parent' in argv else None
pos = [a for i, a in enumerate(argv) if not a.startswith('--') and (i == 0 or argv[i - 1] != '--parent')]
KERNELS = ('k_preprocess', 'k_preprocess_bw')
FRAMES = 10


def body(antialiasing):
    """One process: 3 warm-up frames, then FRAMES timed training frames of one side.  Runs in whichever tree the script lies in (the parent has no flag)."""
    import torch
    import bench
    from nerficg_amd import _lib
    dev = torch.device('cuda', 0)
    gs = bench.build_gs_scene(dev)
    t, rast, H, W = gs['tensors'], gs['rast'], gs['h'], gs['w']
    g_rgb = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) - 0.5
    kw = {'antialiasing': True} if antialiasing else {}

    def frame():
        a = {k: v.detach().requires_grad_(True) for k, v in t.items()}
        image, _ = rast(means3D=a['means3D'], means2D=torch.zeros_like(a['means3D'], requires_grad=True), opacities=a['opacities'], shs=a['shs'],
                        scales=a['scales'], rotations=a['rotations'], **kw)
        image.backward(g_rgb)

    for _ in range(3):
        frame()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(FRAMES):
        frame()
    e1.record()
    e1.synchronize()
    with _lib.stage_timer() as st:
        for _ in range(FRAMES):
            frame()
        torch.cuda.synchronize()
    out = {k: round(tot / FRAMES * 1e3, 2) for k, (tot, cnt) in st.by_name().items() if k in KERNELS}   # us per frame
    out['forward_backward_ms'] = round(e0.elapsed_time(e1) / FRAMES, 4)
    return out


if BODY:
    print(json.dumps(body('antialiasing' in argv)))
    sys.exit(0)

import numpy as np
import torch

ROUNDS = max(5, int(pos[0])) if pos else 7
OUT = pos[1] if len(pos) > 1 else None
summ = lambda v: dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))
result = {'scene': '1000000 Gaussians, 1297x840', 'rounds': ROUNDS, 'frames_per_round': FRAMES, 'units': 'us per launch; forward_backward_ms in ms'}


def child(tree, *flags):
    r = subprocess.run([sys.executable, str(Path(tree) / 'tools' / 'bench_gs_antialias.py'), '--body', *flags], capture_output=True, text=True, cwd=str(tree), timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f'child in {tree} failed ({r.returncode}): {r.stderr[-400:]}')
    return json.loads(r.stdout.strip().splitlines()[-1])


# 1. with and without the flag, this tree, alternating child processes (one GPU process at a time)
sides = {'default': [], 'antialiasing': []}
for _ in range(ROUNDS):
    sides['default'].append(child(ROOT))
    sides['antialiasing'].append(child(ROOT, 'antialiasing'))
result['flag'] = {side: {k: summ([r[k] for r in runs]) for k in KERNELS + ('forward_backward_ms',)} for side, runs in sides.items()}
# 2. the default path against the parent commit, alternating processes
if PARENT and (Path(PARENT) / 'tools').is_dir():
    here, there = [], []
    body_src = Path(__file__).read_text()
    (Path(PARENT) / 'tools' / 'bench_gs_antialias.py').write_text(body_src)      # the parent has no such tool: the same body, run without the flag
    for _ in range(ROUNDS):
        there.append(child(PARENT))
        here.append(child(ROOT))
    cmp = {}
    for k in KERNELS + ('forward_backward_ms',):
        a, b = summ([r[k] for r in here]), summ([r[k] for r in there])
        cmp[k] = dict(this_tree=a, parent=b, inside_parent_spread=bool(b['min'] <= a['median'] <= b['max']))
    result['default_path_vs_parent'] = cmp
else:
    result['default_path_vs_parent'] = 'skipped: no --parent DIR with a built checkout of the parent commit'
# 3. the 3-D filter, 1 M x 200 views, against the torch loop
from tests import scenes
from tests.gs_antialias_ref import view_block
from nerficg_amd.gaussian_splatting import filter_3d
dev = torch.device('cuda', 0)
P, V = 1_000_000, 200
rng = np.random.default_rng(0)
pts = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(P, 3)).astype(np.float32)).to(dev)
views = np.stack([view_block(np.linalg.inv(scenes.orbit_pose(rng.uniform(0, 6.28), rng.uniform(-0.5, 0.5), 4.0)), 1556.4, 1556.4, 1297, 840) for _ in range(V)])
vt = torch.from_numpy(views).to(dev)


def torch_loop():
    """Mip-Splatting's compute_3D_filter, float32 on the device, with the per-view ratio z / fx."""
    dist = torch.full((P,), 1e5, device=dev)
    valid_any = torch.zeros(P, dtype=torch.bool, device=dev)
    for v in range(V):
        m, (fx, fy, W, H) = vt[v, :16].reshape(4, 4), vt[v, 16:].tolist()
        cam = pts @ m[:3, :3].T + m[:3, 3]
        z = cam[:, 2]
        x, y = cam[:, 0] / z.clamp_min(0.001) * fx + W / 2, cam[:, 1] / z.clamp_min(0.001) * fy + H / 2
        valid = (z > 0.2) & (x >= -0.15 * W) & (x <= 1.15 * W) & (y >= -0.15 * H) & (y <= 1.15 * H)
        dist = torch.where(valid, torch.minimum(dist, z / fx), dist)
        valid_any |= valid
    dist[~valid_any] = dist[valid_any].max()
    return dist * (0.2 ** 0.5)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, summ(ms)


a, ta = timed(lambda: filter_3d(pts, vt))
b, tb = timed(torch_loop)
result['filter3d_1M_x_200_views_ms'] = dict(nrc_gs_filter3d=ta, torch_loop=tb, max_relative_difference=float(((a - b).abs() / b).max()))
print(json.dumps(result))
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(result, indent=1))
