#!/usr/bin/env python3
"""tools/bench_bilateral_grid.py [repeats] [out.json] [--parent DIR] [--profile] -- the bilateral-grid colour correction (nerficg_amd.bilateral_grid, C ABI
group 28) on the MI355X: grid (8, 16, 16), N = 200 grids, at the two 3DGS frame sizes.

  slice      forward alone and forward + backward (gradients to the image and the grids) as the fused node, as the module's tensor formula and as the
             grid_sample statement in f32, interleaved in one process: replays of a captured graph of each (the device's share; 10 replays per sample) and
             eager calls (host launch cost included), medians with their spread (min .. max) over `repeats` samples (default 15) after 3 warm-up rounds
  tv         forward + backward at N = 200, fused against the tensor statement, the same way
  kernels    the library's stage timer around eager calls: each kernel's time against its byte model -- 24 B per pixel forward, 36 B per pixel plus the
             partial windows (written once, read once) backward, 2 x 4 B per grid float for each TV kernel -- and the reduction at N = 200 against N = 1
             (what the zero-fill of the other 199 slices of d_grids costs)
  step       the 3DGS optimisation step of tools/bench_gs_step.py (1 M Gaussians) without and with the grid in the loop (slice before the loss, 10 tv_loss,
             the grids' own Adam group), alternating blocks of 20 iterations in one process; with --parent DIR (a checkout of the parent commit with its
             library built) tools/bench_gs_step.py of both trees in alternating processes
--profile: eight eager iterations of slice and TV, forward and backward, at 1297 x 840 and nothing else (for rocprofv3).  Writes the JSON (default profiles/r33_bilateral_grid.json)."""
import json
import statistics
import subprocess
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from nerficg_amd import _lib
from nerficg_amd.bilateral_grid import BilateralGrid, slice as bg_slice, tensor_formula, total_variation_loss, tv_formula

args = [a for a in sys.argv[1:] if not a.startswith('--')]
repeats = int(args[0]) if args else 15
out_path = Path(args[1]) if len(args) > 1 else ROOT / 'profiles' / 'r33_bilateral_grid.json'
parent = Path(sys.argv[sys.argv.index('--parent') + 1]) if '--parent' in sys.argv else None
profile = '--profile' in sys.argv
dev = torch.device('cuda', 0)
N, L, GH, GW = 200, 8, 16, 16
PER_SAMPLE = 10
LUMA = (0.299, 0.587, 0.114)


def grid_sample_statement(grids, rgb, idx):
    """The same operation on interior inputs as tensor operations around grid_sample: rgb (3, H, W), idx an int."""
    _, H, W = rgb.shape
    u = ((torch.arange(W, device=rgb.device, dtype=rgb.dtype) + 0.5) / W)[None, :].expand(H, W)
    v = ((torch.arange(H, device=rgb.device, dtype=rgb.dtype) + 0.5) / H)[:, None].expand(H, W)
    g = LUMA[0] * rgb[0] + LUMA[1] * rgb[1] + LUMA[2] * rgb[2]
    coords = torch.stack([2 * u - 1, 2 * v - 1, 2 * g - 1], -1)[None, None]
    A = torch.nn.functional.grid_sample(grids[idx][None], coords, mode='bilinear', align_corners=True, padding_mode='border')[0, :, 0]      # (12, H, W)
    M = A.reshape(3, 4, H, W)
    return (M[:, :3] * rgb[None]).sum(1) + M[:, 3]


def timed(fn, n=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def summary(ts):
    return dict(median_us=round(statistics.median(ts), 2), min_us=round(min(ts), 2), max_us=round(max(ts), 2), samples=len(ts))


def interleaved(calls, n_per_sample):
    """calls: {name: callable}; medians and spreads of `repeats` samples per name, the names taken in turn."""
    times = {k: [] for k in calls}
    for r in range(repeats + 3):
        for k, f in calls.items():
            t = timed(f, n_per_sample)
            if r >= 3:
                times[k].append(t)
    return {k: summary(v) for k, v in times.items()}


def capture(fn):
    """A captured graph of fn, or None where a statement cannot be captured (its eager figures remain)."""
    try:
        return _capture(fn)
    except RuntimeError as e:
        print('not capturable:', str(e).splitlines()[0])
        torch.cuda.synchronize()
        return None


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def bench_slice(w, h, result):
    gen = torch.Generator(device=dev).manual_seed(0)
    grids = (BilateralGrid(N, GW, GH, L).grids.detach().to(dev) + 0.1 * torch.randn(N, 12, L, GH, GW, device=dev, generator=gen)).requires_grad_(True)
    rgb = (0.02 + 0.96 * torch.rand(3, h, w, device=dev, generator=gen)).requires_grad_(True)
    d_out = torch.randn(3, h, w, device=dev, generator=gen)
    idx = 17
    paths = dict(fused=bg_slice, tensor=tensor_formula, grid_sample=grid_sample_statement)

    def fw(f):
        with torch.no_grad():
            return f(grids, rgb, idx)

    def fwbw(f):
        f(grids, rgb, idx).backward(d_out)
        grids.grad = rgb.grad = None

    with torch.no_grad():   # the three statements agree (f32, interior inputs up to pixels within rounding of a vertex)
        ref = fw(bg_slice)
        result[f'{w}x{h}']['max_abs_difference_to_fused'] = {k: float((fw(f) - ref).abs().max()) for k, f in paths.items() if k != 'fused'}
    for what, run in (('forward', fw), ('forward_backward', fwbw)):
        graphs = {k: capture(lambda f=f: run(f)) for k, f in paths.items()}
        result[f'{w}x{h}'][what] = dict(graph=interleaved({k: g.replay for k, g in graphs.items() if g is not None}, PER_SAMPLE),
                                        eager=interleaved({k: (lambda f=f: run(f)) for k, f in paths.items()}, PER_SAMPLE))
    # per-kernel times (stage timer, eager) against the byte models
    lib = _lib.load()
    ws_floats = int(lib.nrc_bilagrid_ws_floats(N, L, GH, GW, h, w))
    per = {}
    grids1 = grids.detach()[:1].clone().requires_grad_(True)
    for label, g, i in (('N200', grids, idx), ('N1', grids1, 0)):
        acc = {}
        for r in range(repeats + 3):
            with _lib.stage_timer() as t:
                bg_slice(g, rgb, i).backward(d_out)
            g.grad = rgb.grad = None
            if r >= 3:
                for name, ms in t.stages:
                    acc.setdefault(name, []).append(ms * 1e3)
        per[label] = {k: summary(v) for k, v in acc.items()}
    px = w * h
    E = 12 * L * GH * GW
    model = dict(k_bilagrid_slice=24 * px, k_bilagrid_slice_bw=36 * px + 4 * ws_floats, k_bilagrid_reduce_N200=4 * ws_floats + 4 * N * E, k_bilagrid_reduce_N1=4 * ws_floats + 4 * E)
    result[f'{w}x{h}']['kernels'] = dict(stage_timer=per, byte_model=model, workspace_floats=ws_floats,
                                         achieved_GBps={'k_bilagrid_slice': round(model['k_bilagrid_slice'] / per['N200']['k_bilagrid_slice']['median_us'] / 1e3, 1),
                                                        'k_bilagrid_slice_bw': round(model['k_bilagrid_slice_bw'] / per['N200']['k_bilagrid_slice_bw']['median_us'] / 1e3, 1),
                                                        'k_bilagrid_reduce_N200': round(model['k_bilagrid_reduce_N200'] / per['N200']['k_bilagrid_reduce']['median_us'] / 1e3, 1)},
                                         zero_fill_of_199_slices_us=round(per['N200']['k_bilagrid_reduce']['median_us'] - per['N1']['k_bilagrid_reduce']['median_us'], 2))


def bench_tv(result):
    gen = torch.Generator(device=dev).manual_seed(1)
    grids = (BilateralGrid(N, GW, GH, L).grids.detach().to(dev) + 0.1 * torch.randn(N, 12, L, GH, GW, device=dev, generator=gen)).requires_grad_(True)

    def run(f):
        f(grids).backward()
        grids.grad = None

    paths = dict(fused=total_variation_loss, tensor=tv_formula)
    graphs = {k: capture(lambda f=f: run(f)) for k, f in paths.items()}
    acc = {}
    for r in range(repeats + 3):
        with _lib.stage_timer() as t:
            run(total_variation_loss)
        if r >= 3:
            for name, ms in t.stages:
                acc.setdefault(name, []).append(ms * 1e3)
    floats = grids.numel()
    per = {k: summary(v) for k, v in acc.items()}
    result['tv_N200'] = dict(graph=interleaved({k: g.replay for k, g in graphs.items() if g is not None}, PER_SAMPLE), eager=interleaved({k: (lambda f=f: run(f)) for k, f in paths.items()}, PER_SAMPLE),
                             kernels=dict(stage_timer=per, byte_model={'k_bilagrid_tv': 4 * floats, 'k_bilagrid_tv_bw': 8 * floats},
                                          achieved_GBps={'k_bilagrid_tv': round(4 * floats / per['k_bilagrid_tv']['median_us'] / 1e3, 1),
                                                         'k_bilagrid_tv_bw': round(8 * floats / per['k_bilagrid_tv_bw']['median_us'] / 1e3, 1)}),
                             value_difference=abs(float(total_variation_loss(grids)) - float(tv_formula(grids))))


def make_step():
    import bench
    from tests import scenes
    from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera, render_image_training, training_loss
    sc = scenes.gs_random_scene(1_000_000, seed=0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g = Gaussians(T(sc['means3D']), torch.log(T(sc['scales'])), T(sc['rotations']), torch.logit(T(sc['opacities']).clamp(1e-4, 1 - 1e-4))[:, None].contiguous(),
                  T(sc['shs'][:, :1]), T(sc['shs'][:, 1:]))
    g.training_setup(training_cameras_extent=4.5)
    cam = PerspectiveCamera(bench.GS_W, bench.GS_H, 1.2 * bench.GS_W, 1.2 * bench.GS_W, background_color=torch.zeros(3, device=dev))
    target = torch.rand(3, bench.GS_H, bench.GS_W, device=dev)
    poses = [torch.from_numpy(np.asarray(scenes.orbit_pose(0.8 + 0.7 * i, 0.35, 4.5), dtype=np.float32)).to(dev) for i in range(8)]
    bg = BilateralGrid(N, GW, GH, L).to(dev)
    bg_opt = torch.optim.Adam(bg.parameters(), lr=2e-3, eps=1e-15)

    def step(i, with_grid):
        out = render_image_training(g, cam, poses[i % 8])
        if with_grid:
            loss = training_loss(bg(out['rgb'], i % N), target) + 10 * bg.tv_loss()
        else:
            loss = training_loss(out['rgb'], target)
        loss.backward()
        with torch.no_grad():
            g.add_densification_stats(out['viewspace_points'], out['radii'])
        g.optimizer.step(); g.optimizer.zero_grad()
        if with_grid:
            bg_opt.step(); bg_opt.zero_grad()
    return step


def bench_step(result):
    import time
    step = make_step()
    for i in range(3):
        step(i, False), step(i, True)
    times = {False: [], True: []}
    for r in range(5):
        for with_grid in (False, True):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(20):
                step(i, with_grid)
            torch.cuda.synchronize()
            times[with_grid].append((time.perf_counter() - t0) / 20 * 1e6)
    result['gs_step_1M'] = dict(without_grid=summary(times[False]), with_grid=summary(times[True]), iterations_per_sample=20,
                                note='us per optimisation step (host clock around 20 steps ending in a synchronise), alternating blocks in one process')
    if parent is not None:
        runs = {'tree': [], 'parent': []}
        for r in range(3):
            for name, root in (('tree', ROOT), ('parent', parent)):
                out = subprocess.run([sys.executable, str(root / 'tools' / 'bench_gs_step.py'), '1000000', '40'], capture_output=True, text=True, timeout=300, check=True).stdout
                runs[name].append(float(out.strip().splitlines()[-1].split(':')[-1].split()[0]) * 1e3)
        result['gs_step_1M_default_path_vs_parent'] = dict(tree=summary(runs['tree']), parent=summary(runs['parent']),
                                                           note='tools/bench_gs_step.py 1000000 40 of both checkouts, alternating processes, us per step')


if profile:
    gen = torch.Generator(device=dev).manual_seed(0)
    grids = (BilateralGrid(N, GW, GH, L).grids.detach().to(dev) + 0.1 * torch.randn(N, 12, L, GH, GW, device=dev, generator=gen)).requires_grad_(True)
    rgb = (0.02 + 0.96 * torch.rand(3, 840, 1297, device=dev, generator=gen)).requires_grad_(True)
    d_out = torch.randn(3, 840, 1297, device=dev, generator=gen)
    for i in range(8):
        bg_slice(grids, rgb, 17).backward(d_out)
        total_variation_loss(grids).backward()
        grids.grad = rgb.grad = None
    torch.cuda.synchronize()
    sys.exit(0)
result = {'_meta': dict(tool='tools/bench_bilateral_grid.py', device=torch.cuda.get_device_name(0), grid=[L, GH, GW], n_grids=N, repeats=repeats,
                        calls_per_sample=PER_SAMPLE, times='us per call; median, min, max over the samples')}
for w, h in ((1297, 840), (1600, 1060)):
    result[f'{w}x{h}'] = {}
    bench_slice(w, h, result)
bench_tv(result)
bench_step(result)
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(result, indent=1))
print(json.dumps(result, indent=1))
