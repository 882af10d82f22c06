"""The fused InstantNGP frame entered with a caller's own rays (InstantNGPRenderer.render_rays_fused, nrc_ngp_render_count_rays).

  1. a row-major image of rays gives the camera path's picture bit for bit (generate_rays and the camera path's own ray are first shown to be the
     same bits, from the frame's ray_od workspace);
  2. which tile a ray sits in, and with which neighbours, does not change its result (plain list, permuted list);
  3. list lengths that leave lanes / waves of the count pass without a ray;
  4. rays no pinhole produces, against the op-by-op ray-list path and the CPU oracle chain (tolerances: tests/test_gpu_render_parity.py);
  5. a list that misses the box altogether (the rows == 0 branches);
  6. routing through render_rays(fused=...) and the fallback of a non-default grid layout.
"""
import numpy as np
import pytest
import torch

import oracle
from tests import scenes
from tests.test_gpu_garden_parity import garden_model, inside_pose
from tests.test_gpu_render_parity import assert_depth_follows_the_oracle, make_camera, make_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = ('rgb', 'alpha', 'depth')
POSES = ((0.7, 0.4), (2.9, -0.6))


def _keep(out):
    """the results are views of the renderer's workspace: copies survive the next frame"""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _rays_of(cam, c2w):
    from nerficg_amd.raygen import generate_rays
    r = generate_rays(cam.width, cam.height, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, c2w, want_direction=False)
    return r['origin'], r['view_direction']


@pytest.fixture(scope='module', params=['default', 'three cascades, exponential steps'])
def scene(request):
    """(model, renderer, pose of (theta, phi)); the camera pictures of case 1 are rendered once per (size, pose) and shared"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    if request.param == 'default':
        model = make_model()
        return model, InstantNGPRenderer(model), lambda p: scenes.orbit_pose(p[0], p[1], scenes.LEGO_RADIUS), {}
    model = garden_model()
    assert model.cascades == 3
    return model, InstantNGPRenderer(model, EXPONENTIAL_STEPS=True), lambda p: inside_pose(p[0], p[1]), {}


def _camera_picture(scene, w, h, pose):
    """render_image_fused(camera, c2w), single pass, with its statistics and the rays the count pass derived (from the ray_od workspace)"""
    model, renderer, pose_of, cache = scene
    if (w, h, pose) not in cache:
        cam = make_camera(w, h, bg=(1.0, 0.5, 0.25))
        c2w = pose_of(pose)
        ref = _keep(renderer.render_image_fused(cam, c2w, return_stats=True, early_termination=False))
        ws = next(iter(renderer._fused_ws.values()))
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        tile = torch.from_numpy(((ys // 8) * ((w + 7) // 8) + xs // 8).reshape(-1)).to(DEV)
        lane = torch.from_numpy(((ys % 8) * 8 + xs % 8).reshape(-1)).to(DEV)
        od = ws['ray_od'].reshape(-1, 6, 64)[tile, :, lane].clone()     # (H*W, 6): o - centre, d of every pixel
        cache[(w, h, pose)] = cam, c2w, ref, od
    return cache[(w, h, pose)]


# ------------------------------------------------------------------------------------------------ 1. the camera path's picture
@pytest.mark.parametrize('pose', POSES)
@pytest.mark.parametrize('w,h', [(40, 32), (37, 21)])   # 37 x 21: partial tiles on both edges
def test_an_image_of_rays_is_the_camera_picture_bit_for_bit(scene, w, h, pose):
    model, renderer, _, _ = scene
    cam, c2w, ref, od = _camera_picture(scene, w, h, pose)
    origin, view_direction = _rays_of(cam, c2w)
    # the premise: generate_rays (group 5) and the camera path's in-kernel ray are the same bits
    assert torch.equal(origin - model.center, od[:, :3]) and torch.equal(view_direction, od[:, 3:])
    assert ref['n_samples'] > 10 * w * h and (ref['alpha'] > 1e-3).float().mean().item() > 0.2   # a picture, not a background
    for et in (False, True, 'auto'):
        want = _keep(renderer.render_image_fused(cam, c2w, return_stats=True, early_termination=et))
        _same(want, ref, ('camera path', et))
        got = renderer.render_rays_fused(origin, view_direction, cam, image_shape=(h, w), early_termination=et, return_stats=True)
        _same(got, want, et)
        assert (got['n_rows'], got['n_samples']) == (want['n_rows'], want['n_samples']) == (ref['n_rows'], ref['n_samples']), et
    with pytest.raises(RuntimeError, match='image_shape'):
        renderer.render_rays_fused(origin, view_direction, cam, image_shape=(h, w + 1))


# ------------------------------------------------------------------------------------------------ 2. tile membership, 3. tails
@pytest.fixture(scope='module')
def listed(scene):
    """the 37 x 21 picture's rays as a plain list: (rays, the camera picture, the list's result)"""
    _, renderer, _, _ = scene
    cam, c2w, ref, _ = _camera_picture(scene, 37, 21, POSES[0])
    origin, view_direction = _rays_of(cam, c2w)
    flat = _keep(renderer.render_rays_fused(origin, view_direction, cam, return_stats=True))
    return cam, origin, view_direction, ref, flat


def test_tile_membership_does_not_change_a_ray(scene, listed):
    _, renderer, _, _ = scene
    cam, origin, view_direction, ref, flat = listed
    _same(flat, ref, 'list')
    assert flat['n_samples'] == ref['n_samples']
    perm = torch.randperm(origin.shape[0], generator=torch.Generator().manual_seed(11)).to(DEV)
    for et in (False, True):
        shuffled = renderer.render_rays_fused(origin[perm], view_direction[perm], cam, early_termination=et, return_stats=True)
        back = {k: torch.empty_like(shuffled[k]) for k in KEYS}
        for k in KEYS:
            back[k][perm] = shuffled[k]
        _same(back, ref, ('permuted', et))
        assert shuffled['n_samples'] == ref['n_samples']


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])   # empty lanes of a tile; 257: a fifth tile alone in the second workgroup of four waves
def test_list_tails(scene, listed, n):
    _, renderer, _, _ = scene
    cam, origin, view_direction, _, flat = listed
    got = renderer.render_rays_fused(origin[:n], view_direction[:n], cam)
    assert got['rgb'].shape == (n, 3) and got['alpha'].shape == (n,) and got['depth'].shape == (n,)
    _same(got, {k: flat[k][:n] for k in KEYS}, n)


def test_an_empty_list(scene):
    _, renderer, _, _ = scene
    cam = make_camera(8, 8)
    got = renderer.render_rays_fused(torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV), cam)
    assert got['rgb'].shape == (0, 3) and got['alpha'].shape == (0,) and got['depth'].shape == (0,)


# ------------------------------------------------------------------------------------------------ 4. rays no pinhole produces
def _odd_rays():
    """(origin, view_direction, misses): an equirectangular fan from outside the box, rays that start inside it, rays that miss it, axis-parallel
    rays with exact zero components inside and outside the slabs.  Unit directions, float32."""
    rng = np.random.default_rng(5)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    # fan: equal steps of longitude / latitude around the direction from the eye to the box centre (48 x 28 rays, 60 x 44 degrees)
    eye = np.array([0.9, -0.55, 0.35])
    fwd = -eye / np.linalg.norm(eye)
    right = unit(np.cross(fwd, [0.0, 0.0, 1.0])[None])[0]
    up = np.cross(right, fwd)
    lon, lat = np.meshgrid(np.radians(np.linspace(-30, 30, 48)), np.radians(np.linspace(-22, 22, 28)))
    fan = (np.cos(lat) * np.cos(lon))[..., None] * fwd + (np.cos(lat) * np.sin(lon))[..., None] * right + np.sin(lat)[..., None] * up
    fan = fan.reshape(-1, 3)
    o = [np.broadcast_to(eye, fan.shape)]
    d = [fan]
    miss = [np.zeros(len(fan), bool)]
    # 64 rays from inside the box, any direction
    o.append(rng.uniform(-0.3, 0.3, (64, 3)))
    d.append(unit(rng.normal(size=(64, 3))))
    miss.append(np.zeros(64, bool))
    # 64 rays that miss: from outside, pointing away from the centre (within 60 degrees of the outward direction)
    away = unit(rng.normal(size=(64, 3)))
    o.append(away * rng.uniform(1.0, 2.0, (64, 1)))
    d.append(unit(away + 0.5 * rng.uniform(-1, 1, (64, 3))))
    miss.append(np.ones(64, bool))
    # 8 axis-parallel rays: exact zeros in two components; the first of each pair runs inside the other two slabs, the second outside one of them
    axis_o = np.array([[-1.3, 0.1037, -0.0521], [-1.3, 0.7013, -0.0521], [0.0713, 1.4, 0.1291], [0.0713, 1.4, -0.6507],
                       [0.2029, -0.1483, -1.2], [-0.5831, -0.1483, -1.2], [1.1, -0.0379, 0.0467], [1.1, -0.0379, 0.5519]])
    axis_d = np.array([[1, 0, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, 1], [-1, 0, 0], [-1, 0, 0]], dtype=np.float64)
    o.append(axis_o)
    d.append(axis_d)
    miss.append(np.array([False, True] * 4))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32), np.concatenate(miss)


def _oracle_rays(model, cam, origin, view_direction):
    """the CPU chain of tests/test_gpu_render_parity.py::_oracle_image for a list of rays: box test -> near / far clamp -> march -> query ->
    composite with the early-out -> finalise"""
    o = origin - model.center.cpu().numpy()
    d = view_direction
    half = np.float32(model.SCALE)
    _, ht, _ = oracle.ray_aabb_intersect(o, d, np.zeros((1, 3), np.float32), np.full((1, 3), half, np.float32), 1)
    hits = ht[:, 0].copy()
    hits[:, 0] = np.maximum(hits[:, 0], np.float32(cam.near_plane))
    hits[:, 1] = np.minimum(hits[:, 1], np.float32(cam.far_plane))
    bf = model.occupancy_bitfield.cpu().numpy()
    rays_a, xyzs, dirs, deltas, ts, counter = oracle.raymarching_train(o, d, hits, bf, model.cascades, float(half), 0.0, np.zeros(len(o), np.float32), 128, 1024)
    pd = model.encoding_xyz.params.detach().half().float().cpu().numpy()
    pc = model.color_mlp_with_encoding.params.detach().half().float().cpu().numpy()
    x01 = (xyzs - (-half)) / (np.float32(2) * half)
    grid_kw = {k: model.encoding_xyz.grid_cfg[k] for k in ('n_levels', 'log2_hashmap_size', 'base_resolution', 'per_level_scale')}
    sig, rgb, _ = oracle.ngp_query(x01, dirs, pd[:3072], pc, pd[3072:].reshape(-1, 2), **grid_kw)
    _, alpha, depth, col, _ = oracle.composite_train_fw(sig, rgb, deltas, ts, rays_a, 1e-4)
    alpha = np.clip(alpha, 0, 1)
    T = 1 - alpha
    col = np.clip(col + T[:, None] * cam.background_color.numpy()[None], 0, 1)
    depth = np.where(T < 1, depth / np.where(alpha > 0, alpha, 1), 0)
    return col, alpha, depth, int(counter[0]), float(ts.max())


def test_rays_no_pinhole_produces_against_the_ray_list_path_and_the_oracle():
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    model = make_model()
    renderer = InstantNGPRenderer(model)
    cam = make_camera(8, 8, bg=(1.0, 0.5, 0.25))   # depth range and background only
    o_np, d_np, miss = _odd_rays()
    assert 1400 <= len(o_np) <= 1600 and (d_np[-8:] == 0).sum() == 16
    origin, view_direction = torch.from_numpy(o_np).to(DEV), torch.from_numpy(d_np).to(DEV)
    ref = renderer.render_rays(origin, view_direction, cam, train_mode=False)
    got = _keep(renderer.render_rays_fused(origin, view_direction, cam, return_stats=True))
    o_rgb, o_alpha, o_depth, o_total, t_far = _oracle_rays(model, cam, o_np, d_np)
    assert got['n_samples'] == o_total   # the same sample set
    # against the op-by-op path
    for name, a, b, tol in (('rgb', got['rgb'], ref['rgb'], 2e-3), ('alpha', got['alpha'], ref['alpha'], 1e-3)):
        diff = (a - b).abs()
        print(f'ray-list path, {name}: max {diff.max().item():.3e} mean {diff.mean().item():.3e}')
        assert diff.max().item() <= tol and diff.mean().item() <= tol / 10, (name, diff.max().item(), diff.mean().item())
    hit = ref['alpha'] > 1e-3
    assert (got['depth'] - ref['depth']).abs()[hit].max().item() <= 5e-3
    # against the CPU oracle
    rgb, alpha, depth = (got[k].cpu().numpy() for k in KEYS)
    print(f'oracle: rgb max {np.abs(rgb - o_rgb).max():.3e} mean {np.abs(rgb - o_rgb).mean():.3e} alpha max {np.abs(alpha - o_alpha).max():.3e}')
    np.testing.assert_allclose(rgb, o_rgb, rtol=0, atol=2e-3)
    np.testing.assert_allclose(alpha, o_alpha, rtol=0, atol=1e-3)
    assert np.abs(rgb - o_rgb).mean() <= 2e-4
    assert_depth_follows_the_oracle(depth, o_depth, o_alpha, 1e-3, t_far)
    # the rays that miss: exactly the background, nothing else
    bg = cam.background_color.numpy()
    assert (o_alpha[miss] == 0).all() and (rgb[miss] == bg).all() and (alpha[miss] == 0).all() and (depth[miss] == 0).all()
    # ... and the others are not trivial: the fan both hits and misses, the rays from inside and the axis-parallel ones in the slabs hit
    n_fan = len(o_np) - 136
    assert 0.2 < (o_alpha[:n_fan] > 1e-3).mean() < 0.8 and (o_alpha[n_fan:n_fan + 64] > 1e-3).mean() > 0.4
    assert (o_alpha[-8:][~miss[-8:]] > 1e-3).all()


# ------------------------------------------------------------------------------------------------ 5. nothing hit
def test_a_list_that_misses_the_box(scene):
    _, renderer, _, _ = scene
    cam = make_camera(8, 8, bg=(0.25, 0.5, 1.0))
    away = torch.nn.functional.normalize(torch.randn(130, 3, generator=torch.Generator().manual_seed(2)), dim=1).to(DEV)
    for et in (False, True, 'auto'):
        got = renderer.render_rays_fused(away * 5.0, away, cam, early_termination=et, return_stats=True)   # (5 / sqrt 3 > 2: outside the larger box too)
        assert (got['n_rows'], got['n_samples']) == (0, 0)
        assert got['rgb'].shape == (130, 3) and torch.equal(got['rgb'], cam.background_color.to(DEV).expand(130, 3))
        assert not got['alpha'].any() and not got['depth'].any()


# ------------------------------------------------------------------------------------------------ 6. routing and fallback
def test_render_rays_routes_to_the_fused_frame_on_request(scene, listed):
    _, renderer, _, _ = scene
    cam, origin, view_direction, _, flat = listed
    bg = torch.tensor([0.2, 0.9, 0.4])
    want = _keep(renderer.render_rays_fused(origin, view_direction, cam, custom_bg_color=bg))
    assert not torch.equal(want['rgb'], flat['rgb'])   # (the background is the caller's)
    _same(renderer.render_rays(origin, view_direction, cam, train_mode=False, custom_bg_color=bg, fused=True), want, 'fused=True')
    # the default stays the op-by-op path
    step_growth = 1 / 256 if renderer.EXPONENTIAL_STEPS else 0.0
    o, d, span = renderer.clip_rays(origin, view_direction, cam)
    _same(renderer.render_rays(origin, view_direction, cam, train_mode=False, custom_bg_color=bg), renderer._render_ray_list(o, d, span, bg.to(DEV), step_growth),
          'fused=False')


def test_a_non_default_grid_layout_falls_back_to_the_ray_list_path():
    from nerficg_amd.instant_ngp import InstantNGPModel, InstantNGPRenderer
    model = InstantNGPModel(HASHGRID_N_LEVELS=8, HASHGRID_N_FEATURES_PER_LEVEL=4, RANDOM_SEED=5, device=DEV)
    with torch.no_grad():
        model.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.35, 1)).to(DEV))
    renderer = InstantNGPRenderer(model)
    cam = make_camera(24, 16)
    origin, view_direction = _rays_of(cam, scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS))
    want = renderer.render_rays(origin, view_direction, cam, train_mode=False)
    assert (want['alpha'] > 0).any()
    _same(renderer.render_rays_fused(origin, view_direction, cam), want, 'render_rays_fused')
    _same(renderer.render_rays(origin, view_direction, cam, train_mode=False, fused=True), want, 'fused=True')
