#!/usr/bin/env python3
"""tools/bench_ray_list.py -- the 800x800 bench frame through the three doors of the fused InstantNGP pipeline:

  camera       render_image_fused(camera, c2w): the count pass derives every ray from the pinhole (and once more with the encoder's default brick
               instead of the one chosen from the pose: the ray forms have no pose, so that is the like-for-like yardstick of the count pass);
  image rays   render_rays_fused(origin, view_direction, image_shape=(H, W)): the same rays read from memory (nerficg_amd.raygen.generate_rays, made
               outside the timed window -- they are the caller's input), tiled as the camera path's 8x8 pixel blocks;
  ray strips   render_rays_fused without image_shape: the same rays as a plain list, 64 consecutive rays = a 64x1 pixel strip per tile.

ms per frame over the bench poses (host clock around frames that end in a device synchronise), the forms alternating inside every round so that they
share whatever else the machine is doing; per form the median, fastest and slowest ROUND.  The three pictures of a pose are checked to be identical.
Usage: python tools/bench_ray_list.py [--rounds 5] [--frames 20] [--json PATH]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import bench  # noqa: E402
from nerficg_amd import _lib  # noqa: E402
from nerficg_amd.raygen import generate_rays  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--frames', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--json', type=str, default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), 'bench_ray_list.py measures on the GPU; there is no fallback'
dev = torch.device('cuda', 0)
model, renderer, cam, poses = bench.build_scene(dev)
W, H = cam.width, cam.height
n_poses = args.warmup + args.frames
assert len(poses) >= n_poses, (len(poses), n_poses)
rays = []
for p in poses[:n_poses]:
    r = generate_rays(W, H, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, p, device=dev, want_direction=False)
    rays.append((r['origin'], r['view_direction']))



def camera_default_brick(i):
    """the camera path with the encoder's default brick, which is what the ray forms run with (they have no pose to choose one from)"""
    renderer.POSE_ENCODER_SHAPE = False
    _lib.load().nrc_ngp_set_encoder_shape(-1, -1)
    try:
        return renderer.render_image_fused(cam, poses[i], return_stats=True)
    finally:
        renderer.POSE_ENCODER_SHAPE = True


forms = {
    'camera': lambda i: renderer.render_image_fused(cam, poses[i], return_stats=True),
    'camera, default brick': camera_default_brick,
    'image rays': lambda i: renderer.render_rays_fused(*rays[i], cam, image_shape=(H, W), return_stats=True),
    'ray strips': lambda i: renderer.render_rays_fused(*rays[i], cam, return_stats=True),
}

# the same picture three times
keep = lambda out: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
ref = keep(forms['camera'](args.warmup))
identical = {}
for name in ('image rays', 'ray strips'):
    out = forms[name](args.warmup)
    identical[name] = all(torch.equal(out[k], ref[k]) for k in ('rgb', 'alpha', 'depth')) and out['n_samples'] == ref['n_samples']


def timed(fn) -> float:
    for i in range(args.warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.frames):
        fn(args.warmup + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.frames * 1e3


ms = {name: [] for name in forms}
for _ in range(args.rounds):
    for name, fn in forms.items():
        ms[name].append(timed(fn))

result = {'width': W, 'height': H, 'rounds': args.rounds, 'frames_per_round': args.frames, 'samples_of_the_checked_pose': int(ref['n_samples']),
          'identical_to_camera_picture': identical, 'ms_per_frame': {}}
base = statistics.median(ms['camera'])
for name, v in ms.items():
    med = statistics.median(v)
    result['ms_per_frame'][name] = {'median': round(med, 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'rounds': [round(x, 4) for x in v],
                                    'mrays_per_s': round(W * H / med * 1e-3, 2), 'vs_camera': round(med / base, 4)}
    print('%-21s %.3f ms median (%.3f .. %.3f over %d rounds) = %.2f Mrays/s, %.3f x camera' % (name, med, min(v), max(v), args.rounds, W * H / med * 1e-3, med / base))
print('identical pictures:', identical)
print(json.dumps(result))
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(json.dumps(result, indent=1) + '\n')
