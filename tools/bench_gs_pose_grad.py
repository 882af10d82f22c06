#!/usr/bin/env python3
"""tools/bench_gs_pose_grad.py -- what the camera gradient costs: the backward pass of the 1 M-Gaussian 1297x840 frame (bench.build_gs_scene, the README's 3DGS frame)
without and with camera_grad=True, the two legs alternating inside every round.

Per round and leg: `--frames` forward + backward passes, the backward of each between two HIP events (ms per backward = the mean over the frames).  Reported: the
median over `--rounds` rounds, fastest and slowest round, every round; and, from the library's stage timer over `--frames` more frames, the ms per frame of the
kernels of the backward (k_render_bw, k_pose_bw, k_pose_finish, k_preprocess_bw).  On a tree without the flag (the parent commit) only the plain leg runs, so the
same file measures both sides of an A/B on one lease.  Result: one JSON document (default profiles/r15_gs_pose_grad.json)."""
import argparse
import inspect
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gaussians', type=int, default=1_000_000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r15_gs_pose_grad.json'))
    args = ap.parse_args()
    from nerficg_amd import _lib
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device('cuda', 0)
    gs = bench.build_gs_scene(dev, args.gaussians)
    rs = gs['rast'].raster_settings
    has_flag = 'camera_grad' in inspect.signature(GaussianRasterizer.forward).parameters
    rasterizers = {'plain': (gs['rast'], {})}
    pose = {}
    if has_flag:
        pose = {k: getattr(rs, k).detach().clone().requires_grad_(True) for k in ('viewmatrix', 'projmatrix', 'campos')}
        rasterizers['camera_grad'] = (GaussianRasterizer(rs._replace(**pose)), {'camera_grad': True})
    t = gs['tensors']
    g = torch.rand(3, gs['h'], gs['w'], device=dev)

    def frame(leg, events=None):
        rast, kw = rasterizers[leg]
        for p in pose.values():        # (a fresh .grad every frame: no accumulation launches inside the timed backward)
            p.grad = None
        leaves = {k: v.detach().requires_grad_(True) for k, v in t.items()}
        m2d = torch.zeros_like(leaves['means3D'], requires_grad=True)
        color, _ = rast(means3D=leaves['means3D'], means2D=m2d, opacities=leaves['opacities'], shs=leaves['shs'], scales=leaves['scales'],
                        rotations=leaves['rotations'], **kw)
        if events is not None:
            events[0].record()
        color.backward(g)
        if events is not None:
            events[1].record()

    for leg in rasterizers:            # warm-up: list sizes, allocator, the kept record buffer
        for _ in range(4):
            frame(leg)
    torch.cuda.synchronize()
    rounds = {leg: [] for leg in rasterizers}
    for _ in range(args.rounds):
        for leg in rasterizers:
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.frames)]
            for ev in pairs:
                frame(leg, ev)
            torch.cuda.synchronize()
            rounds[leg].append(sum(a.elapsed_time(b) for a, b in pairs) / args.frames)
    kernels = {}
    for leg in rasterizers:
        with _lib.stage_timer() as st:
            for _ in range(args.frames):
                frame(leg)
        kernels[leg] = {k: round(tot / args.frames, 5) for k, (tot, cnt) in st.by_name().items() if k in ('k_render_bw', 'k_pose_bw', 'k_pose_finish', 'k_preprocess_bw')}
    out = {'tool': 'tools/bench_gs_pose_grad.py', 'gaussians': args.gaussians, 'width': gs['w'], 'height': gs['h'], 'rounds': args.rounds, 'frames_per_round': args.frames,
           'unit': 'ms per backward pass (HIP events around .backward())', 'device': torch.cuda.get_device_name(0), 'legs': {}, 'kernel_ms_per_frame': kernels}
    for leg, vals in rounds.items():
        s = sorted(vals)
        out['legs'][leg] = {'median': round(s[len(s) // 2], 5), 'fastest': round(s[0], 5), 'slowest': round(s[-1], 5), 'rounds': [round(v, 5) for v in vals]}
    if has_flag:
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in pose.values())
        out['extra_ms'] = round(out['legs']['camera_grad']['median'] - out['legs']['plain']['median'], 5)
    text = json.dumps(out, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
