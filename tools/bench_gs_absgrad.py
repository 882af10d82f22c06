#!/usr/bin/env python3
"""tools/bench_gs_absgrad.py [rounds=9] [out.json] [--kernel-stats stats.csv] | --trace-body -- what absgrad=True adds to a 3DGS training frame.

Scene: the bench's 1 M synthetic Gaussians at 1297x840 (bench.build_gs_scene), the sizes tools/bench_gs_features.py uses.  In ONE process, alternating per
round (at least five rounds): the rasterizer's forward + backward without the flag and with it, HIP events around the whole call and around the backward alone;
median and spread (min .. max) of each side, as the project's measuring practice asks -- a difference counts only when it exceeds the two spreads together.

k_render_bw's own times come from a SEPARATE run under the profiler (counters and traces never share a run with the event timing):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/bench_gs_absgrad.py --trace-body
runs 2 warm-up and 10 measured frames of each side; `--kernel-stats DIR/.../*_kernel_stats.csv` on the timing run folds the per-instance averages into the
JSON.  The bar the flag is held to: the added time stays below one k_render_bw launch of the frame without the flag -- what a stand-alone replay kernel
would cost at the least.  Prints one JSON object; writes it to out.json when given (profiles/r28_gs_absgrad.json)."""
import csv
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import bench

argv = sys.argv[1:]
TRACE_BODY = '--trace-body' in argv
STATS = argv[argv.index('--kernel-stats') + 1] if '--kernel-stats' in argv else None
pos = [a for i, a in enumerate(argv) if not a.startswith('--') and (i == 0 or argv[i - 1] != '--kernel-stats')]
ROUNDS = max(5, int(pos[0])) if pos else 9
OUT = pos[1] if len(pos) > 1 else None
dev = torch.device('cuda', 0)
gs = bench.build_gs_scene(dev)
t, rast, P, W, H = gs['tensors'], gs['rast'], gs['n'], gs['w'], gs['h']
gen = torch.Generator(device=dev).manual_seed(0)
g_rgb = torch.rand(3, H, W, device=dev, generator=gen) - 0.5


def frame(absgrad, events=None):
    a = {k: v.detach().requires_grad_(True) for k, v in t.items()}
    m2 = torch.zeros_like(a['means3D'], requires_grad=True)
    image, _ = rast(means3D=a['means3D'], means2D=m2, opacities=a['opacities'], shs=a['shs'], scales=a['scales'], rotations=a['rotations'], absgrad=absgrad)
    if events is not None:
        events[0].record()
    image.backward(g_rgb)
    if events is not None:
        events[1].record()
    assert hasattr(m2, 'absgrad') == absgrad
    return m2


if TRACE_BODY:
    for flag in (False, True):
        for _ in range(12):
            frame(flag)
        torch.cuda.synchronize()
    sys.exit(0)

for flag in (False, True):
    frame(flag)
torch.cuda.synchronize()
ms = {(flag, part): [] for flag in (False, True) for part in ('forward_backward', 'backward')}
for _ in range(ROUNDS):
    for flag in (False, True):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        frame(flag, events=(e[1], e[2]))
        e[3].record()
        e[3].synchronize()
        ms[(flag, 'forward_backward')].append(e[0].elapsed_time(e[3]))
        ms[(flag, 'backward')].append(e[1].elapsed_time(e[2]))
summ = lambda v: dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
result = {'scene': f'{P} Gaussians, {W}x{H}', 'rounds': ROUNDS}
for part in ('forward_backward', 'backward'):
    plain, flagged = summ(ms[(False, part)]), summ(ms[(True, part)])
    spreads = (plain['max_ms'] - plain['min_ms']) + (flagged['max_ms'] - flagged['min_ms'])
    result[part] = dict(plain=plain, absgrad=flagged, added_ms=round(flagged['median_ms'] - plain['median_ms'], 4), two_spreads_ms=round(spreads, 4))
m2 = frame(True)
a, s = m2.absgrad[:, :2], m2.grad[:, :2].abs()
live = a > 0
result['median_signed_over_abs'] = round(float((s[live] / a[live]).median()), 4)
if STATS:
    inst = {}
    for row in csv.DictReader(open(STATS)):
        m = re.search(r'k_render_bw<(\w+), (\w+)>', row['Name'])
        if m:
            inst[f'k_render_bw<{m.group(1)}, {m.group(2)}>'] = dict(calls=int(row['Calls']), average_us=round(float(row['AverageNs']) / 1e3, 2),
                                                                    min_us=round(float(row['MinNs']) / 1e3, 2), max_us=round(float(row['MaxNs']) / 1e3, 2))
    result['k_render_bw'] = inst
    base, flagged = inst.get('k_render_bw<false, false>'), inst.get('k_render_bw<false, true>')
    if base and flagged:
        result['k_render_bw_added_us'] = round(flagged['average_us'] - base['average_us'], 2)
        result['bar_one_plain_k_render_bw_launch_us'] = base['average_us']
        result['added_backward_time_below_the_bar'] = bool(result['backward']['added_ms'] * 1e3 < base['average_us'])
print(json.dumps(result))
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(result, indent=1))
