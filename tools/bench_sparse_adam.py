#!/usr/bin/env python3
"""tools/bench_sparse_adam.py [repeats] [--out FILE] [--sizes N,N] [--profile] -- the visibility-masked Adam launch (nrc_adam_step_rows_multi, csrc/adam_rows.hip)
against the dense launch (nrc_adam_step_multi) on the six 3DGS model tensors (59 floats per Gaussian), P = 1 M and 6 M.

Per size, before any timing and in the same process: (a) an all-visible mask leaves the bits of the dense step, (b) a random 20 % mask leaves every invisible row
of p, m, v untouched.  Then, per mask, the dense and the masked launch ALTERNATE (the dense launch streams 16 B x 59 x P between two masked ones, so a small
visible set cannot stay in the 256 MiB Infinity Cache from one repeat to the next), each launch between its own pair of HIP events; medians over `repeats`
(default 21, at least 9) and the spread = 90th - 10th percentile, min and max.  Masks: random rows at 5 / 20 / 50 / 100 %, contiguous runs (period 4096 rows)
at the same fractions, and the real radii of the eight orbit poses of tools/bench_gs_step.py.  Two byte models per mask, computed from the mask:
lower bound 28 * sum(width) * P_visible + mask bytes; line-granular: the 128-B lines of each of the seven streams (p, g, m, v read; p, m, v written) that hold
a visible element, + mask bytes.  Finally the whole optimisation step as tools/bench_gs_step.py runs it, with and without sparse_adam.
--profile: P = 1 M, the random 20 % mask only, masked launches only (for rocprofv3: the counters then belong to ONE known mask); prints its byte models."""
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

import bench
from nerficg_amd import _lib
from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera, render_image_training, training_loss
from tests import scenes

args = [a for a in sys.argv[1:]]
out_file = args[args.index('--out') + 1] if '--out' in args else None
sizes = [int(s) for s in args[args.index('--sizes') + 1].split(',')] if '--sizes' in args else [1_000_000, 6_000_000]
profile = '--profile' in args
positional = [a for k, a in enumerate(args) if not a.startswith('--') and (k == 0 or args[k - 1] not in ('--out', '--sizes'))]
repeats = max(9, int(positional[0])) if positional else 21

dev = torch.device('cuda', 0)
lib = _lib.load()
WIDTHS = (3, 3, 45, 1, 3, 4)            # positions, f_dc, f_rest, opacities, scales, rotations
LRS = (1.6e-4 * 4.5, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
cast = lambda a: ctypes.cast(a, ctypes.c_void_p)


class Tensors:
    """p, g, m, v of the six tensors and the host argument arrays of both entry points."""

    def __init__(self, P, seed=0):
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.P = P
        self.p = [torch.randn(P, w, device=dev, generator=gen) for w in WIDTHS]
        self.g = [torch.randn(P, w, device=dev, generator=gen) * 1e-3 for w in WIDTHS]
        self.m = [torch.randn(P, w, device=dev, generator=gen) * 1e-3 for w in WIDTHS]
        self.v = [torch.rand(P, w, device=dev, generator=gen) * 1e-6 for w in WIDTHS]
        n = len(WIDTHS)
        self._keep = []                  # the host arrays behind the cast pointers

        def keep(a):
            self._keep.append(a)
            return cast(a)
        arr = lambda ts: keep((ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]))
        self.ptrs = [arr(ts) for ts in (self.p, self.g, self.m, self.v)]
        self.sizes = keep((ctypes.c_int64 * n)(*[t.numel() for t in self.p]))
        self.widths = keep((ctypes.c_int32 * n)(*WIDTHS))
        self.lrs = keep((ctypes.c_float * n)(*LRS))
        bc = 1.0 - BETA1 ** 10, 1.0 - BETA2 ** 10
        self.bc1, self.bc2 = keep((ctypes.c_float * n)(*[bc[0]] * n)), keep((ctypes.c_float * n)(*[bc[1]] * n))
        self.stream = _lib.stream_of(self.p[0])

    def dense(self):
        _lib.check(lib.nrc_adam_step_multi(len(WIDTHS), *self.ptrs, self.sizes, self.lrs, self.bc1, self.bc2, BETA1, BETA2, EPS, 0.0, 0, self.stream), 'adam_step_multi')

    def masked(self, mask):
        _lib.check(lib.nrc_adam_step_rows_multi(len(WIDTHS), *self.ptrs, self.widths, self.P, _lib.ptr(mask), 1 if mask.dtype == torch.int32 else 0, self.lrs, self.bc1,
                                                self.bc2, BETA1, BETA2, EPS, 0.0, 0, self.stream), 'adam_step_rows_multi')

    def state(self):
        return [t.clone() for ts in (self.p, self.m, self.v) for t in ts]

    def restore(self, saved):
        for t, s in zip([t for ts in (self.p, self.m, self.v) for t in ts], saved):
            t.copy_(s)


def bits(t):
    return t.view(torch.int32)


def checks(T):
    saved = T.state()
    T.dense()
    dense = T.state()
    T.restore(saved)
    T.masked(torch.ones(T.P, dtype=torch.int32, device=dev))
    all_visible_equals_dense = all(torch.equal(bits(a), bits(b)) for a, b in zip(T.state(), dense))
    T.restore(saved)
    mask = torch.rand(T.P, device=dev) < 0.2
    poisoned = [g.clone() for g in T.g]
    for g in T.g:
        g[~mask] = float('nan')
    T.masked(mask)
    after = T.state()
    invisible_untouched = all(torch.equal(bits(a)[~mask], bits(b)[~mask]) for a, b in zip(after, saved))
    visible_moved = all(bool((bits(a)[mask] != bits(b)[mask]).any()) for a, b in zip(after[:6], saved[:6]))
    for g, s in zip(T.g, poisoned):
        g.copy_(s)
    T.restore(saved)
    torch.cuda.synchronize()
    return dict(all_visible_equals_dense_bit_for_bit=all_visible_equals_dense, invisible_rows_untouched_at_20_percent=invisible_untouched, visible_rows_moved=visible_moved)


def byte_models(mask_bool, mask_bytes):
    """(lower bound, line-granular) bytes of a masked launch; tensors taken as 128-B aligned (the allocator's blocks are)."""
    rows = torch.nonzero(mask_bool).flatten().to(torch.int64)
    n_vis = int(rows.numel())
    lower = 28 * sum(WIDTHS) * n_vis + mask_bytes
    lines = 0
    for w in WIDTHS:
        first = (rows * w * 4) // 128
        last = ((rows * w + w) * 4 - 1) // 128
        prev_last = torch.cat([first.new_full((1,), -1), last[:-1]])
        lines += int((last - torch.maximum(first, prev_last + 1) + 1).clamp(min=0).sum())
    return lower, 7 * 128 * lines + mask_bytes


def quantiles(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), spread_p10_p90_ms=float(np.quantile(a, 0.9) - np.quantile(a, 0.1)), min_ms=float(a[0]), max_ms=float(a[-1]))


def time_pair(T, mask, n):
    dense_ms, masked_ms = [], []
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for k in range(n + 3):      # three warm-up rounds
        a, b, c, d = ev(), ev(), ev(), ev()
        a.record(); T.dense(); b.record()
        c.record(); T.masked(mask); d.record()
        torch.cuda.synchronize()
        if k >= 3:
            dense_ms.append(a.elapsed_time(b)); masked_ms.append(c.elapsed_time(d))
    return dense_ms, masked_ms


def model(P):
    sc = scenes.gs_random_scene(P, seed=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return Gaussians(t(sc['means3D']), torch.log(t(sc['scales'])), t(sc['rotations']), torch.logit(t(sc['opacities']).clamp(1e-4, 1 - 1e-4))[:, None].contiguous(),
                     t(sc['shs'][:, :1]), t(sc['shs'][:, 1:]))


cam = PerspectiveCamera(bench.GS_W, bench.GS_H, 1.2 * bench.GS_W, 1.2 * bench.GS_W, background_color=torch.zeros(3, device=dev))
poses = [torch.from_numpy(np.asarray(scenes.orbit_pose(0.8 + 0.7 * i, 0.35, 4.5), dtype=np.float32)).to(dev) for i in range(8)]


def whole_step(P, sparse, iters=16):
    g = model(P)
    g.training_setup(training_cameras_extent=4.5, sparse_adam=sparse)
    target = torch.rand(3, bench.GS_H, bench.GS_W, device=dev)

    def step(i):
        out = render_image_training(g, cam, poses[i % 8])
        training_loss(out['rgb'], target).backward()
        with torch.no_grad():
            g.add_densification_stats(out['viewspace_points'], out['radii'])
        g.optimizer_step(out['radii'] if sparse else None); g.optimizer.zero_grad()

    for i in range(8):
        step(i)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(iters):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


if profile:
    T = Tensors(1_000_000)
    mask = (torch.rand(T.P, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.2)
    lower, lines = byte_models(mask, T.P)
    for _ in range(repeats):
        T.masked(mask)
    torch.cuda.synchronize()
    print(json.dumps(dict(profile=True, P=T.P, mask='random 20 %', launches=repeats, visible_fraction=float(mask.float().mean()), lower_bound_bytes=lower,
                          line_granular_bytes=lines, line_granular_read_bytes=(lines - T.P) * 4 // 7 + T.P, line_granular_write_bytes=(lines - T.P) * 3 // 7)))
    sys.exit(0)

result = dict(device=torch.cuda.get_device_name(0), repeats=repeats, widths=list(WIDTHS), spread_definition='90th - 10th percentile of the launch times of the row',
              sizes={})
for P in sizes:
    T = Tensors(P)
    entry = dict(checks=checks(T), masks=[])
    print(f'P = {P}: checks {entry["checks"]}', flush=True)
    if not all(entry['checks'].values()):
        result['sizes'][str(P)] = entry
        print(json.dumps(result))
        sys.exit('bench_sparse_adam: a check failed, nothing is timed')
    gen = torch.Generator(device=dev).manual_seed(2)
    rows = torch.arange(P, device=dev)
    masks = []
    for pct in (5, 20, 50, 100):
        masks.append((f'random {pct} %', (torch.rand(P, device=dev, generator=gen) < pct / 100.0) if pct < 100 else torch.ones(P, dtype=torch.bool, device=dev)))
    for pct in (5, 20, 50, 100):
        masks.append((f'runs {pct} % (period 4096)', (rows % 4096) < round(40.96 * pct)))
    g = model(P)
    for i, pose in enumerate(poses):
        masks.append((f'orbit pose {i} radii', render_image_training(g, cam, pose)['radii'].clone()))
    del g
    for name, mask in masks:
        vis = mask > 0 if mask.dtype == torch.int32 else mask
        lower, lines = byte_models(vis, P * mask.element_size())
        d, m = time_pair(T, mask, repeats)
        dq, mq = quantiles(d), quantiles(m)
        row = dict(mask=name, mask_dtype=str(mask.dtype).replace('torch.', ''), visible_fraction=float(vis.float().mean()), lower_bound_bytes=lower, line_granular_bytes=lines,
                   dense=dq, masked=mq, masked_minus_dense_ms=mq['median_ms'] - dq['median_ms'],
                   dense_bytes=28 * sum(WIDTHS) * P, dense_TBps=28 * sum(WIDTHS) * P / dq['median_ms'] / 1e9,
                   masked_TBps_of_line_granular=lines / mq['median_ms'] / 1e9)
        entry['masks'].append(row)
        print(f"  {name:28s} visible {row['visible_fraction']:.3f}  dense {dq['median_ms']:.4f} ms (spread {dq['spread_p10_p90_ms']:.4f})  masked {mq['median_ms']:.4f} ms "
              f"(spread {mq['spread_p10_p90_ms']:.4f})  lower {lower / 1e6:.1f} MB  lines {lines / 1e6:.1f} MB  {row['masked_TBps_of_line_granular']:.2f} TB/s of the line model", flush=True)
    del T
    torch.cuda.empty_cache()
    entry['whole_step_ms'] = dict(dense=whole_step(P, False), sparse_adam=whole_step(P, True))
    print(f"  whole optimisation step: dense {entry['whole_step_ms']['dense']:.3f} ms, sparse_adam {entry['whole_step_ms']['sparse_adam']:.3f} ms", flush=True)
    torch.cuda.empty_cache()
    result['sizes'][str(P)] = entry
text = json.dumps(result, indent=1)
if out_file:
    Path(out_file).parent.mkdir(parents=True, exist_ok=True)
    Path(out_file).write_text(text)
print(json.dumps(result))
