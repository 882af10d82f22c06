"""The image encoder reads the hashed levels that follow the block view's dense levels (levels 5-8 of the shipped grid) through a vertex view
(include/nerficg_hip.h: nrc_ngp_build_vertex_view -- per level a dense array of the 4-byte fp16 pairs of its vertices in x + R (y + R z) order, R = res + 2;
nrc_ngp_set_encoder_vertex_view / _vertex_levels): four 8-byte loads instead of the hash, four 16-byte loads and a predicated round of four more.  The
view holds COPIES of table entries and the encoder feeds them to the same weights in the same order, so everything here is an equality of bits: the view
against a numpy restatement of the spatial hash, the feature buffer and the pictures with V = 1 .. 4 levels read through the view against V = 0, a view
that follows the parameters, a grid whose first hashed level is too large for a view, and a view that does not outlive a refused call.  The tables are
full-range random fp16 pairs: a U(-1e-4, 1e-4) table would hide a wrong corner."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scenes
from tests.test_gpu_encoder_block_view import _assert_same_frames, _cfg, _frames, _levels, _shipped_grid

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VIEW_LEVELS = (5, 6, 7, 8)      # the shipped grid: res 81 112 154 213, hashed only because (res + 1)^3 just exceeds 2^19


def _vertex_levels(lv, cap=128 << 20):
    """the levels a vertex view holds, restated: the hashed levels behind the leading dense ones (at most 5 of those), at most 4, below `cap` bytes"""
    first = 0
    while first < 5 and first < len(lv) and not lv[first][4]:
        first += 1
    out, nbytes = [], 0
    for l in range(first, min(first + 4, len(lv))):
        if not lv[l][4] or nbytes + 4 * (lv[l][2] + 2) ** 3 > cap:
            break
        out.append(l)
        nbytes += 4 * (lv[l][2] + 2) ** 3
    return out, nbytes


def test_view_holds_the_entries_the_hash_names():
    """vertex (x, y, z) of a view level is table[offset + ((x ^ y 2654435761 ^ z 805459861) & (size - 1))]: every vertex of level 5, a seeded sample of
    100 000 vertices of each further level (the corners x, y, z in {0, R - 1} among them)"""
    from nerficg_amd import _lib
    lib, g = _lib.load(), _shipped_grid()
    lv = _levels(g)
    levels, nbytes = _vertex_levels(lv)
    assert tuple(levels) == VIEW_LEVELS and [lv[l][2] for l in levels] == [81, 112, 154, 213]
    assert int(lib.nrc_ngp_vertex_view_bytes(*_cfg(g))) == nbytes == 4 * (83 ** 3 + 114 ** 3 + 156 ** 3 + 215 ** 3)        # 63.2 MB
    total = lv[-1][0] + lv[-1][1]
    table = torch.from_numpy(np.random.default_rng(11).integers(0, 2 ** 32, size=total, dtype=np.uint32).view(np.int32)).to(DEV)
    view = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.nrc_ngp_build_vertex_view(_lib.ptr(table), *_cfg(g), _lib.ptr(view), _lib.stream_of(view)), 'build')
    got = view.cpu().numpy().view(np.uint32)
    tab = table.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(12)
    first = 0
    for l in levels:
        off, size, res, _, _ = lv[l]
        R = res + 2
        assert size == 1 << 19
        if l == levels[0]:
            v = np.arange(R ** 3, dtype=np.int64)
        else:
            corners = np.array([x + R * (y + R * z) for x in (0, R - 1) for y in (0, R - 1) for z in (0, R - 1)], np.int64)
            v = np.concatenate([corners, rng.integers(0, R ** 3, size=100_000 - 8)])
        x, y, z = (v % R).astype(np.uint64), (v // R % R).astype(np.uint64), (v // (R * R)).astype(np.uint64)
        h = (x ^ (y * np.uint64(2654435761)) ^ (z * np.uint64(805459861))) & np.uint64(size - 1)     # (the low 19 bits of the 32-bit products)
        assert np.array_equal(got[first + v], tab[off + h.astype(np.int64)]), l
        first += R ** 3
    assert first == got.shape[0]


def _special_values(lv, levels):
    """coordinates at which the cell or a weight of a view level steps or sits in the middle: 0, 1, 1 - ulp, k / scale and (k +- 0.5) / scale for cells at
    both ends and in the middle of the level (odd and even ones), and the float32 neighbours of each on either side"""
    vals = [0.0, 1.0]
    for l in levels:
        _, _, res, scale, _ = lv[l]
        for k in sorted({0, 1, 2, res // 2, res // 2 + 1, res - 3, res - 2, res - 1, int(scale)}):
            vals += [v for v in (k / scale, (k - 0.5) / scale, (k + 0.5) / scale) if 0.0 <= v <= 1.0]
    vals = np.asarray(vals, np.float32)
    return np.unique(np.clip(np.concatenate([vals, np.nextafter(vals, np.float32(-1)), np.nextafter(vals, np.float32(2))]), 0.0, 1.0))


@pytest.fixture(scope='module')
def ray_tile():
    """one ray tile of 16 rows (1 024 slots, one block of bricks) for nrc_ngp_encode_samples: ray r starts on the plane (its axis r % 3) = 0 with special
    values on the other two axes and runs along that axis with d = 1, so p = o + t d is exact and a special t puts all three coordinates on special values"""
    from tests.test_gpu_render_parity import make_model
    model = make_model()
    enc = model.encoding_xyz
    lv = _levels(enc.grid_cfg)
    rows, n = 16, 1024
    vals = _special_values(lv, VIEW_LEVELS)
    ends = np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)      # exactly 0, exactly 1, 1 - ulp
    assert 100 < len(vals) < 800 and vals[0] == ends[0] and vals[-1] == ends[1] and vals[-2] == ends[2]
    rng = np.random.default_rng(5)
    o = rng.choice(vals, size=(64, 3)).astype(np.float32)
    for i, e in enumerate(ends):                            # rays 3 .. 11: the two axes across the ray on an end value
        o[3 + 3 * i:6 + 3 * i] = e
    d = np.zeros((64, 3), np.float32)
    o[np.arange(64), np.arange(64) % 3] = 0.0
    d[np.arange(64), np.arange(64) % 3] = 1.0
    ts = rng.choice(vals, size=n).astype(np.float32)
    ts[:len(vals)] = vals                                   # every special value at least once
    holes = np.flatnonzero(rng.random(n) < 0.1)
    ts[holes[holes >= len(vals)]] = -1.0
    for i, e in enumerate(ends):                            # rows 13 .. 15, rays 0 .. 2 (one per axis): the axis along the ray on an end value
        ts[64 * (13 + i):64 * (13 + i) + 3] = e
    live = ts >= 0
    assert (~live).sum() > 20
    pos = o[np.arange(n) % 64] + ts[:, None] * d[np.arange(n) % 64]
    for axis in range(3):
        assert all((pos[live, axis] == e).any() for e in ends), axis
    # what the slots cover, per view level: the cell along the ray's axis is floor(scale t + 0.5)
    for l in VIEW_LEVELS:
        _, _, res, scale, _ = lv[l]
        f = np.float32(scale) * ts[live].astype(np.float64) + 0.5
        clear = np.abs(f - np.round(f)) > 0.01                # (away from a step of the floor: no doubt about the cell)
        gx = np.floor(f[clear]).astype(np.int64)
        top = int(np.floor(np.float32(scale) + 0.5))          # the last cell a position in the box reaches: res - 1 or res - 2
        assert top in (res - 1, res - 2) and gx.max() == top and gx.min() == 0, l
        assert (gx % 2 == 0).sum() > 10 and (gx % 2 == 1).sum() > 10, l
    assert sum(int(np.floor(np.float32(lv[l][3]) + 0.5)) == lv[l][2] - 1 for l in VIEW_LEVELS) >= 3      # cells gx = res - 1 at three of the four levels
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ray_od = np.concatenate([o.T, d.T]).reshape(1, 6, 64)   # per-tile SoA [6][64]
    return enc, rows, n, T(ts), T(ray_od), T(np.zeros(rows, np.int32))


def _encode(ray_tile, levels, view, n_rows=None):
    """nrc_ngp_encode_samples on the ray tile with `levels` levels read through `view` (None: no view is set); returns (code, features)"""
    from nerficg_amd import _lib
    lib = _lib.load()
    enc, rows, n, ts_d, od_d, rt_d = ray_tile
    mn, sz = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    vp = ctypes.c_void_p
    feat = torch.full((n * 64,), 0x3C, dtype=torch.uint8, device=DEV)
    assert lib.nrc_ngp_set_encoder_vertex_levels(levels) == 0
    if view is not None:
        assert lib.nrc_ngp_set_encoder_vertex_view(_lib.ptr(view)) == 0
    rc = lib.nrc_ngp_encode_samples(_lib.ptr(ts_d), _lib.ptr(rt_d), _lib.ptr(od_d), 0, rows if n_rows is None else n_rows, ctypes.cast(mn, vp),
                                    ctypes.cast(sz, vp), _lib.ptr(enc._table16()), *_cfg(enc.grid_cfg), _lib.ptr(feat), None, 0, _lib.stream_of(feat))
    return rc, feat


def test_features_of_one_ray_tile_equal_those_of_the_table_path(ray_tile):
    """positions on and next to cell faces and centres, 0, 1 and 1 - ulp on every axis, odd and even cells, the last cells of the levels, holes -- the
    feature buffer with V = 1 .. 4 is the V = 0 buffer"""
    from nerficg_amd import _lib
    lib = _lib.load()
    enc = ray_tile[0]
    enc._half_params()
    view = enc._vertex_view()
    assert view is not None and view.numel() == int(lib.nrc_ngp_vertex_view_bytes(*_cfg(enc.grid_cfg)))
    try:
        rc, want = _encode(ray_tile, 0, view)
        assert rc == 0
        f16 = want.view(torch.float16)
        assert bool(torch.isfinite(f16).all()) and float(f16.abs().max()) > 0.1        # features of an amplified table, not the fill pattern
        for levels in (1, 2, 3, 4, -1):
            rc, got = _encode(ray_tile, levels, view)
            assert rc == 0 and torch.equal(got, want), levels
    finally:
        lib.nrc_ngp_set_encoder_vertex_levels(-1)
        lib.nrc_ngp_set_encoder_vertex_view(None)


def test_a_view_does_not_outlive_the_call_it_was_set_for(ray_tile):
    """a view of the right size and the WRONG content (zeros) changes the features when it is read -- and is read by nobody after the call it was set for,
    whether that call ran or was refused at validation"""
    from nerficg_amd import _lib
    lib = _lib.load()
    enc = ray_tile[0]
    enc._half_params()
    wrong = torch.zeros_like(enc._vertex_view())
    try:
        rc, want = _encode(ray_tile, 0, None)
        assert rc == 0
        rc, got = _encode(ray_tile, 4, wrong)
        assert rc == 0 and not torch.equal(got, want)                 # the premise: a set view is read
        rc, got = _encode(ray_tile, 4, None)                          # the call above took it
        assert rc == 0 and torch.equal(got, want)
        rc, _ = _encode(ray_tile, 4, wrong, n_rows=-1)                # refused: NRC_ERR_INVALID
        assert rc == -1
        rc, got = _encode(ray_tile, 4, None)
        assert rc == 0 and torch.equal(got, want)
    finally:
        lib.nrc_ngp_set_encoder_vertex_levels(-1)
        lib.nrc_ngp_set_encoder_vertex_view(None)


def _bench_shaped_model(seed=0):
    """the benchmark's scene (sphere of radius 0.35 in the unit box, seeded networks) with a full-range table: U(-2, 2) instead of U(-1e-4, 1e-4)"""
    from tests.test_gpu_render_parity import make_model
    return make_model(seed=seed)


def test_frames_with_the_view_equal_frames_without():
    """64 x 48 pixels through render_image_fused, every form that launches the tiled encoder (single pass, slab order, fixed row capacity, tile shards),
    and the same rays through render_rays_fused: V = 1 .. 4 and the default against V = 0"""
    from nerficg_amd import _lib
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from nerficg_amd.raygen import generate_rays
    from tests.test_gpu_render_parity import make_camera
    lib = _lib.load()
    model, pose = _bench_shaped_model(), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    cam = make_camera(64, 48, bg=(0.2, 0.4, 0.6))
    renderer = InstantNGPRenderer(model)
    n_tiles = renderer.n_image_tiles(cam)
    r = generate_rays(cam.width, cam.height, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, pose, want_direction=False)

    def frames():
        out = _frames(renderer, cam, pose, n_tiles)
        got = renderer.render_rays_fused(r['origin'], r['view_direction'], cam, image_shape=(48, 64), early_termination=False)
        out['ray list'] = {k: got[k].clone() for k in ('rgb', 'alpha', 'depth')}
        return out

    try:
        assert lib.nrc_ngp_set_encoder_vertex_levels(0) == 0
        want = frames()
        assert model.encoding_xyz._vertex_view() is not None
        assert float(want['single pass']['alpha'].max()) > 0.1
        assert torch.equal(want['ray list']['rgb'].reshape(-1, 3), want['single pass']['rgb'].reshape(-1, 3))
        for levels in (1, 2, 3, 4, -1):
            assert lib.nrc_ngp_set_encoder_vertex_levels(levels) == 0
            _assert_same_frames(frames(), want, levels)
    finally:
        lib.nrc_ngp_set_encoder_vertex_levels(-1)


def _picture(renderer, cam, pose, levels=-1):
    """single-pass frame with `levels` hashed levels read through the vertex view (-1: the default, 0: those levels from the table), as copies"""
    from nerficg_amd import _lib
    lib = _lib.load()
    try:
        assert lib.nrc_ngp_set_encoder_vertex_levels(levels) == 0
        out = renderer.render_image_fused(cam, pose, early_termination=False)
        return {k: out[k].clone() for k in ('rgb', 'alpha', 'depth')}
    finally:
        lib.nrc_ngp_set_encoder_vertex_levels(-1)


def test_view_follows_the_parameters():
    """render; an optimizer step; render; an in-place write to entries of levels 5-8 (a version bump); render: every picture is the table path's on the
    parameters of its time, and differs from the one before"""
    from nerficg_amd.apex_optimizers import FusedAdam
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    model = make_model()
    enc = model.encoding_xyz
    cam, pose = make_camera(64, 48), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    renderer = InstantNGPRenderer(model)
    first = _picture(renderer, cam, pose)
    view = enc._vertex_view()
    assert view is not None and enc._vertex_view() is view        # valid from frame to frame
    for k, v in _picture(renderer, cam, pose, levels=0).items():
        assert torch.equal(first[k], v), k
    opt = FusedAdam(model.parameters(), lr=1e-1, eps=1e-15, betas=(0.9, 0.99), adam_w_mode=False)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    second = _picture(renderer, cam, pose)
    for k, v in _picture(renderer, cam, pose, levels=0).items():
        assert torch.equal(second[k], v), ('optimizer step', k)
    assert not torch.equal(second['rgb'], first['rgb'])
    lv = _levels(enc.grid_cfg)
    with torch.no_grad():   # only entries of levels 5-8 change: a stale view would paint the second picture again
        a, b = 3072 + 2 * lv[5][0], 3072 + 2 * (lv[8][0] + lv[8][1])
        enc.params[a:b] *= -1.5
    third = _picture(renderer, cam, pose)
    for k, v in _picture(renderer, cam, pose, levels=0).items():
        assert torch.equal(third[k], v), ('in-place write', k)
    assert not torch.equal(third['rgb'], second['rgb'])


def test_frames_after_a_replayed_optimiser_step_equal_the_table_path():
    """A HIP-graph replay rewrites the fp16 table with no Python in between.  From the recording on, the module has no vertex view (rebuilding 63 MB for every
    frame costs more than it saves): render, replays, render -- the second picture is the table path's on the trained model, and not the first."""
    from nerficg_amd.apex_optimizers import FusedAdam
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    model = make_model()
    enc = model.encoding_xyz
    renderer = InstantNGPRenderer(model)
    cam, pose = make_camera(64, 48), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15, betas=(0.9, 0.99), adam_w_mode=False, capturable=True)
    for p in model.parameters():       # a fixed gradient: every entry moves by about lr per step
        p.grad = torch.ones_like(p)
    opt.step()                         # eager: creates the moments
    first = _picture(renderer, cam, pose)
    assert enc._vertex_view() is not None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    before = enc.params.detach().clone()
    for _ in range(3):
        graph.replay()
    assert not torch.equal(enc.params.detach()[3072:], before[3072:])     # the replays trained the table
    second = _picture(renderer, cam, pose)
    assert enc._vertex_view() is None
    table = _picture(renderer, cam, pose, levels=0)
    assert torch.equal(enc._half_params(), enc.params.detach().half())   # the copy the table path read is current
    for k in first:
        assert torch.equal(second[k], table[k]), k
    assert not torch.equal(second['rgb'], first['rgb'])


def test_a_grid_whose_first_hashed_level_passes_the_cap_has_no_view():
    """base resolution 400: level 0 is hashed (400^3 entries do not fit 2^19) and its 402^3 vertices alone are 260 MB -- no view, and the frames of such a
    model read the table whatever is asked for"""
    from nerficg_amd import _lib
    from nerficg_amd.instant_ngp import InstantNGPModel, InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    lib = _lib.load()
    model = InstantNGPModel(RANDOM_SEED=5, HASHGRID_BASE_RESOLUTION=400, device=DEV)
    enc = model.encoding_xyz
    with torch.no_grad():
        n = enc.params.numel() - 3072
        enc.params[3072:] = ((torch.rand(n, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 2.0).to(DEV)
        model.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.35, 1)).to(DEV))
    lv = _levels(enc.grid_cfg)
    assert lv[0][4] and lv[0][2] == 400 and _vertex_levels(lv) == ([], 0)
    assert int(lib.nrc_ngp_vertex_view_bytes(*_cfg(enc.grid_cfg))) == 0 and int(lib.nrc_ngp_block_view_bytes(*_cfg(enc.grid_cfg))) == 0
    enc._half_params()
    assert enc._vertex_view() is None
    cam, pose = make_camera(64, 48), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    renderer = InstantNGPRenderer(model)
    want = _picture(renderer, cam, pose, levels=0)
    assert float(want['alpha'].max()) > 0.1
    got = _picture(renderer, cam, pose, levels=4)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_the_setter_takes_minus_one_to_four():
    from nerficg_amd import _lib
    lib = _lib.load()
    try:
        for ok in (0, 1, 2, 3, 4, -1):
            assert lib.nrc_ngp_set_encoder_vertex_levels(ok) == 0, ok
        for bad in (-2, 5, 16, 2 ** 31 - 1):
            assert lib.nrc_ngp_set_encoder_vertex_levels(bad) == -1, bad
    finally:
        lib.nrc_ngp_set_encoder_vertex_levels(-1)
