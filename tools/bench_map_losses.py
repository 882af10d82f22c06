#!/usr/bin/env python3
"""tools/bench_map_losses.py [repeats] -- the map regularisers (depth smoothness + alpha entropy on the rasterizer's maps, normalisation included) forward and
backward, as the three launches of nerficg_amd.map_losses.map_regularizer (A) and as the tensor formula (B), at the two 3DGS frame sizes.  Device events
around one forward + backward, A and B interleaved in one process, medians and minima over `repeats` (default 30) after 5 warm-up rounds: once as eager
calls (host launch cost included, as in the training loop) and once as replays of a captured graph of each path (the device's share alone)."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from nerficg_amd.map_losses import map_regularizer, tensor_formula

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device('cuda', 0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


for w, h in ((1297, 840), (1600, 1060)):
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = (0.05 + 0.9 * torch.rand(1, h, w, device=dev, generator=g)).requires_grad_(True)
    depth = ((1 + 4 * torch.rand(1, h, w, device=dev, generator=g)) * alpha.detach()).requires_grad_(True)
    image = torch.rand(1, 3, h, w, device=dev, generator=g).requires_grad_(True)

    def run(f):
        loss = f(depth, alpha, image, 0.1, 0.01, True, False)
        loss.backward()
        depth.grad = alpha.grad = image.grad = None

    paths = (('fused', map_regularizer), ('tensor', tensor_formula))
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _, f in paths:
            run(f)
    torch.cuda.current_stream().wait_stream(side)
    for name, f in paths:
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            run(f)
    times = {(mode, name): [] for mode in ('eager', 'graph') for name, _ in paths}
    for r in range(repeats + 5):
        for name, f in paths:
            for mode, call in (('eager', lambda: run(f)), ('graph', graphs[name].replay)):
                t = timed(call)
                if r >= 5:
                    times[(mode, name)].append(t)
    for (mode, name), ts in times.items():
        print(f'{w}x{h} {mode} {name:6s} forward+backward: median {statistics.median(ts):8.1f} us  min {min(ts):8.1f} us  ({len(ts)} repeats)')
