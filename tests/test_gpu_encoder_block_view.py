"""The image encoder reads the table's leading dense levels through a cell-block view (include/nerficg_hip.h: nrc_ngp_build_block_view -- per cell one
32-byte record with the fp16 pairs of its eight corners; nrc_ngp_set_encoder_block_view / _block_levels): two 16-byte loads of one address instead of
eight gathers.  The view holds COPIES of table entries and the encoder feeds them to the same weights in the same order, so everything here is an
equality of bits: the view against a numpy restatement of the dense index, the feature buffer and the pictures with B = 1 .. 5 levels read through the
view against B = 0, a view that follows the parameters, and grids that have fewer dense levels than asked for -- or none."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scenes

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = ((2, 2), (2, 1), (3, 1))   # the three bricks the renderer chooses from (InstantNGPRenderer._frame_constants)


def _cfg(g):
    return g['n_levels'], g['log2_hashmap_size'], g['base_resolution'], float(g['per_level_scale'])


def _levels(g):
    """(offset, size, res, scale, hashed) per level, restated: scale = base * growth^l - 1, res = ceil(scale) + 1, size = res^3 rounded up to 8 and cut at
    the hash-map size (the offsets are checked against nrc_grid_layout)."""
    from nerficg_amd import _lib
    n = g['n_levels']
    offs = (ctypes.c_uint32 * (n + 1))()
    assert _lib.load().nrc_grid_layout(*_cfg(g), ctypes.cast(offs, ctypes.c_void_p)) == 0
    out = []
    for l in range(n):
        scale = float(np.float32(np.exp2(np.float32(l) * np.log2(np.float32(g['per_level_scale'])))) * np.float32(g['base_resolution']) - np.float32(1))
        res = int(np.ceil(scale)) + 1
        size = min((res ** 3 + 7) // 8 * 8, 1 << g['log2_hashmap_size'])
        assert offs[l + 1] - offs[l] == size, l
        out.append((int(offs[l]), size, res, scale, size < res ** 3))
    return out


def _shipped_grid():
    from nerficg_amd.instant_ngp import InstantNGPModel
    return InstantNGPModel(RANDOM_SEED=3, device=DEV).encoding_xyz.grid_cfg


def test_view_holds_the_entries_of_the_dense_index():
    """every record of every level of the view of a random table: corner k of cell (gx, gy, gz) is entry x + y res + z res^2, wrapped once at `size`,
    clamped to `size - 1`, behind the level's offset -- all cells of levels 0-4, the faces gx, gy, gz in {0, res - 1, res} among them"""
    from nerficg_amd import _lib
    lib, g = _lib.load(), _shipped_grid()
    lv = _levels(g)
    dense = [l for l in lv[:5] if not l[4]]
    assert len(dense) == 5 and lv[5][4]              # the shipped grid: levels 0-4 dense, level 5 hashed
    nbytes = int(lib.nrc_ngp_block_view_bytes(*_cfg(g)))
    assert nbytes == 32 * sum((res + 1) ** 3 for _, _, res, _, _ in dense) == 32 * (17 ** 3 + 24 ** 3 + 32 ** 3 + 44 ** 3 + 60 ** 3)   # res 16 23 31 43 59: 11.29 MB
    total = lv[-1][0] + lv[-1][1]
    table = torch.from_numpy(np.random.default_rng(11).integers(0, 2 ** 32, size=total, dtype=np.uint32).view(np.int32)).to(DEV)
    view = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.nrc_ngp_build_block_view(_lib.ptr(table), *_cfg(g), _lib.ptr(view), _lib.stream_of(view)), 'build')
    got = view.cpu().numpy().view(np.uint32).reshape(-1, 8)
    tab = table.cpu().numpy().view(np.uint32)
    first = 0
    for off, size, res, _, _ in dense:
        r1 = res + 1
        gz, gy, gx = np.meshgrid(np.arange(r1, dtype=np.int64), np.arange(r1, dtype=np.int64), np.arange(r1, dtype=np.int64), indexing='ij')
        want = np.empty((r1 ** 3, 8), np.uint32)
        for k in range(8):
            e = (gx + (k & 1)) + (gy + ((k >> 1) & 1)) * res + (gz + (k >> 2)) * res * res
            e = np.where(e >= size, e - size, e)
            e = np.minimum(e, size - 1)
            want[:, k] = tab[off + e.reshape(-1)]
        assert np.array_equal(got[first:first + r1 ** 3], want), res
        first += r1 ** 3
    assert first == got.shape[0]


def _special_values(lv):
    """coordinates at which the cell or a weight of a dense level steps: 0, 1, k / scale and (k +- 0.5) / scale (the floor of scale p + 0.5 steps at
    the latter), and the float32 neighbours of each on either side"""
    vals = [0.0, 1.0]
    for _, _, res, scale, hashed in lv[:5]:
        if hashed:
            continue
        for k in sorted({0, 1, 2, res // 2, res - 2, res - 1, int(scale)}):
            vals += [v for v in (k / scale, (k - 0.5) / scale, (k + 0.5) / scale) if 0.0 <= v <= 1.0]
    vals = np.asarray(vals, np.float32)
    return np.unique(np.clip(np.concatenate([vals, np.nextafter(vals, np.float32(-1)), np.nextafter(vals, np.float32(2))]), 0.0, 1.0))


@pytest.mark.parametrize('shape', SHAPES)
def test_features_of_one_ray_tile_equal_those_of_the_table_path(shape):
    """nrc_ngp_encode_samples on one ray tile of 16 rows (1 024 slots, one block of bricks): positions on and next to cell faces, 0 and 1, holes --
    the feature buffer with B = 1, 3, 5 is the B = 0 buffer"""
    from nerficg_amd import _lib
    from tests.test_gpu_render_parity import make_model
    lib = _lib.load()
    model = make_model()
    enc = model.encoding_xyz
    g = enc.grid_cfg
    rows, n = 16, 1024
    vals = _special_values(_levels(g))
    assert 100 < len(vals) < n
    rng = np.random.default_rng(5)
    # ray r starts on the plane (its axis r % 3) = 0 with special values on the other two axes and runs along that axis with d = 1: p = o + t d is
    # exact, so a special t puts all three coordinates of the sample on special values
    o = rng.choice(vals, size=(64, 3)).astype(np.float32)
    o[0], o[1], o[2] = 0.0, 1.0, (1.0, 0.0, 1.0)
    d = np.zeros((64, 3), np.float32)
    o[np.arange(64), np.arange(64) % 3] = 0.0
    d[np.arange(64), np.arange(64) % 3] = 1.0
    ts = rng.choice(vals, size=n).astype(np.float32)
    ts[:len(vals)] = vals                                   # every special value at least once
    holes = np.flatnonzero(rng.random(n) < 0.1)
    ts[holes[holes >= len(vals)]] = -1.0
    assert (ts < 0).sum() > 20 and ts[0] == 0.0 and (ts == 1.0).any()
    ray_od = np.concatenate([o.T, d.T]).reshape(1, 6, 64)  # per-tile SoA [6][64]
    row_tile = np.zeros(rows, np.int32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ts_d, od_d, rt_d = T(ts), T(ray_od), T(row_tile)
    mn, sz = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    vp = ctypes.c_void_p
    enc._half_params()
    view = enc._block_view()
    assert view is not None and view.numel() == int(lib.nrc_ngp_block_view_bytes(*_cfg(g)))

    def encode(levels):
        feat = torch.full((n * 64,), 0x3C, dtype=torch.uint8, device=DEV)
        assert lib.nrc_ngp_set_encoder_block_levels(levels) == 0
        assert lib.nrc_ngp_set_encoder_block_view(_lib.ptr(view)) == 0
        _lib.check(lib.nrc_ngp_encode_samples(_lib.ptr(ts_d), _lib.ptr(rt_d), _lib.ptr(od_d), 0, rows, ctypes.cast(mn, vp), ctypes.cast(sz, vp),
                                              _lib.ptr(enc._table16()), *_cfg(g), _lib.ptr(feat), None, 0, _lib.stream_of(feat)), 'encode')
        return feat

    try:
        assert lib.nrc_ngp_set_encoder_shape(*shape) == 0
        want = encode(0)
        f16 = want.view(torch.float16)
        assert bool(torch.isfinite(f16).all()) and float(f16.abs().max()) > 0.1        # features of an amplified table, not the fill pattern
        for levels in (1, 3, 5):
            assert torch.equal(encode(levels), want), (shape, levels)
        # the view is taken by the call it was set for: the next call reads the table (a null view where a level asks for one would return zeros)
        assert lib.nrc_ngp_set_encoder_block_levels(5) == 0
        feat = torch.full((n * 64,), 0x3C, dtype=torch.uint8, device=DEV)
        _lib.check(lib.nrc_ngp_encode_samples(_lib.ptr(ts_d), _lib.ptr(rt_d), _lib.ptr(od_d), 0, rows, ctypes.cast(mn, vp), ctypes.cast(sz, vp),
                                              _lib.ptr(enc._table16()), *_cfg(g), _lib.ptr(feat), None, 0, _lib.stream_of(feat)), 'encode')
        assert torch.equal(feat, want)
    finally:
        lib.nrc_ngp_set_encoder_block_levels(-1)
        lib.nrc_ngp_set_encoder_block_view(None)
        lib.nrc_ngp_set_encoder_shape(-1, -1)


def _frames(renderer, cam, pose, n_tiles):
    """the frame forms that launch k_grid_encode<SRC_TILED>: single pass, slab order, fixed row capacity, a shard behind tile 0"""
    out = {}
    forms = {'single pass': dict(early_termination=False), 'slab order': dict(early_termination=True),
             'shard': dict(early_termination=False, tile_begin=n_tiles // 3, n_tiles=n_tiles // 2),
             'shard, slab order': dict(early_termination=True, tile_begin=n_tiles // 3, n_tiles=n_tiles // 2)}
    for name, kw in forms.items():
        r = renderer.render_image_fused(cam, pose, return_stats=True, **kw)
        assert r['n_samples'] > 0, name
        out[name] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items() if k in ('rgb', 'alpha', 'depth', 'n_samples', 'n_rows')}
    cap = int(1.2 * out['single pass']['n_rows']) + 8
    r = renderer.render_image_fused(cam, pose, row_capacity=cap)
    out['row capacity'] = {'rgb': r['rgb'].clone(), 'alpha': r['alpha'].clone(), 'depth': r['depth'].clone(), 'n_samples': r['counter'].tolist()[1]}
    return out


def _assert_same_frames(got, want, where):
    for name in want:
        for k, v in want[name].items():
            same = torch.equal(got[name][k], v) if torch.is_tensor(v) else got[name][k] == v
            assert same, (where, name, k)


@pytest.mark.parametrize('scene', ['unit box', 'scale 2, three cascades'])
def test_frames_with_the_view_equal_frames_without(scene):
    """60 x 44 pixels (partial edge tiles) of a seeded random model through render_image_fused, every form; the scale-2 model takes the division in
    fetch_pos and has four dense levels, so the default B = 5 stops at 4 there"""
    from nerficg_amd import _lib
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    lib = _lib.load()
    if scene == 'unit box':
        model, pose, kw = make_model(), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS), {}
    else:
        from tests.test_gpu_garden_parity import garden_model
        model, pose, kw = garden_model(), scenes.orbit_pose(1.3, 0.25, 1.15), dict(EXPONENTIAL_STEPS=True)
        assert model.cascades == 3
    cam = make_camera(60, 44, bg=(0.2, 0.4, 0.6))
    renderer = InstantNGPRenderer(model, **kw)
    n_tiles = renderer.n_image_tiles(cam)
    try:
        assert lib.nrc_ngp_set_encoder_block_levels(0) == 0
        want = _frames(renderer, cam, pose, n_tiles)
        assert float(want['single pass']['alpha'].max()) > 0.1
        for levels in (-1, 2):
            assert lib.nrc_ngp_set_encoder_block_levels(levels) == 0
            _assert_same_frames(_frames(renderer, cam, pose, n_tiles), want, (scene, levels))
    finally:
        lib.nrc_ngp_set_encoder_block_levels(-1)


def test_view_follows_the_parameters():
    """render, change the grid parameters in place, render again: the second picture is a fresh renderer's on the changed model, not the first"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    model = make_model()
    cam, pose = make_camera(60, 44), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    renderer = InstantNGPRenderer(model)
    first = {k: v.clone() for k, v in renderer.render_image_fused(cam, pose, early_termination=False).items() if k in ('rgb', 'alpha', 'depth')}
    view = model.encoding_xyz._block_view()
    assert model.encoding_xyz._block_view() is view        # valid from frame to frame
    lv = _levels(model.encoding_xyz.grid_cfg)
    with torch.no_grad():   # only entries of the dense levels 0-4 change: a stale view would paint the first picture again
        n_dense = lv[5][0] * 2
        model.encoding_xyz.params[3072:3072 + n_dense] *= -1.5
    second = _picture(renderer, cam, pose)
    fresh = InstantNGPRenderer(model).render_image_fused(cam, pose, early_termination=False)
    table = _picture(renderer, cam, pose, levels=0)     # (the view lives in the model: a fresh renderer shares it, the table path does not)
    for k in first:
        assert torch.equal(second[k], fresh[k]) and torch.equal(second[k], table[k]), k
    assert not torch.equal(second['rgb'], first['rgb'])


def _picture(renderer, cam, pose, levels=-1):
    """single-pass frame with `levels` dense levels read through the view (-1: the default, 0: every level from the table), as copies"""
    from nerficg_amd import _lib
    lib = _lib.load()
    try:
        assert lib.nrc_ngp_set_encoder_block_levels(levels) == 0
        out = renderer.render_image_fused(cam, pose, early_termination=False)
        return {k: out[k].clone() for k in ('rgb', 'alpha', 'depth')}
    finally:
        lib.nrc_ngp_set_encoder_block_levels(-1)


@pytest.mark.parametrize('recording', ['graphed iteration', 'own capture of the optimizer step'])
def test_view_follows_a_replayed_optimiser_step(recording):
    """A HIP-graph replay rewrites the parameters and their fp16 copy through raw pointers with no Python in between -- nothing bumps a version on its
    own.  Validation render, replays, validation render: the second picture is the table path's on the trained model (which reads the fp16 copy the
    replayed Adam kernel keeps current), and not the first.  Both the library's GraphedIteration and a caller's own torch.cuda.graph."""
    from nerficg_amd.apex_optimizers import FusedAdam
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    model = make_model()
    renderer = InstantNGPRenderer(model)
    cam, pose = make_camera(60, 44), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15, betas=(0.9, 0.99), adam_w_mode=False, capturable=True)
    if recording == 'graphed iteration':
        from nerficg_amd.graphs import instant_ngp_iteration
        from tests.test_gpu_graphs import _rays
        tcam, o, d = _rays()
        n = 2048
        scaler = torch.amp.GradScaler(init_scale=128.0, growth_interval=10 ** 6)
        step = instant_ngp_iteration(model, InstantNGPRenderer(model), opt, scaler, tcam, n_rays=n, sample_capacity=400_000)
        batch = dict(origin=o[:n].contiguous(), view_direction=d[:n].contiguous(), rgb=torch.full((n, 3), 0.5, device=DEV))
        step(**batch)                      # eager
        step(**batch)                      # recorded, first replay
        assert step.recorded
        replay = lambda: step(**batch)
    else:
        for p in model.parameters():       # a fixed gradient: every entry moves by about lr per step
            p.grad = torch.ones_like(p)
        opt.step()                         # eager: creates the moments
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
        replay = graph.replay
    first = _picture(renderer, cam, pose)
    view = model.encoding_xyz._block_view()
    assert view is not None
    before = model.encoding_xyz.params.detach().clone()
    for _ in range(3):
        replay()
    assert not torch.equal(model.encoding_xyz.params.detach()[3072:], before[3072:])     # the replays trained the table
    second = _picture(renderer, cam, pose)
    table = _picture(renderer, cam, pose, levels=0)
    assert torch.equal(model.encoding_xyz._half_params(), model.encoding_xyz.params.detach().half())   # the copy the table path read is current
    for k in first:
        assert torch.equal(second[k], table[k]), (recording, k)
    assert not torch.equal(second['rgb'], first['rgb'])


@pytest.mark.parametrize('log2_T,view_levels', [(14, 2), (11, 0), (1, 0)])
def test_grids_with_fewer_dense_levels_render_as_without_a_view(log2_T, view_levels):
    """a hash map of 2^14 entries leaves levels 0-1 dense (16^3, 23^3), level 2 is hashed: B = 5 reads two levels through the view, the rest from the
    table; with 2^11 entries level 0 is hashed and there is no view at all; with 2 entries per level the level offsets are no multiples of 4 entries
    either.  Same pictures as B = 0."""
    from nerficg_amd import _lib
    from nerficg_amd.instant_ngp import InstantNGPModel, InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    lib = _lib.load()
    model = InstantNGPModel(RANDOM_SEED=5, HASHGRID_LOG2_SIZE=log2_T, device=DEV)
    with torch.no_grad():
        n = model.encoding_xyz.params.numel() - 3072
        model.encoding_xyz.params[3072:] = ((torch.rand(n, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 2.0).to(DEV)
        model.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.35, 1)).to(DEV))
    lv = _levels(model.encoding_xyz.grid_cfg)
    assert [l[4] for l in lv[:view_levels + 1]] == [False] * view_levels + [True]
    assert int(lib.nrc_ngp_block_view_bytes(*_cfg(model.encoding_xyz.grid_cfg))) == 32 * sum((l[2] + 1) ** 3 for l in lv[:view_levels])
    model.encoding_xyz._half_params()
    assert (model.encoding_xyz._block_view() is None) == (view_levels == 0)
    cam, pose = make_camera(60, 44), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    renderer = InstantNGPRenderer(model)
    try:
        assert lib.nrc_ngp_set_encoder_block_levels(0) == 0
        want = {k: v.clone() for k, v in renderer.render_image_fused(cam, pose, early_termination=False).items() if k in ('rgb', 'alpha', 'depth')}
        assert float(want['alpha'].max()) > 0.1
        assert lib.nrc_ngp_set_encoder_block_levels(5) == 0
        got = renderer.render_image_fused(cam, pose, early_termination=False)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    finally:
        lib.nrc_ngp_set_encoder_block_levels(-1)


def test_the_setter_takes_minus_one_to_five():
    from nerficg_amd import _lib
    lib = _lib.load()
    try:
        for ok in (0, 1, 2, 3, 4, 5, -1):
            assert lib.nrc_ngp_set_encoder_block_levels(ok) == 0, ok
        for bad in (-2, 6, 16, 2 ** 31 - 1):
            assert lib.nrc_ngp_set_encoder_block_levels(bad) == -1, bad
    finally:
        lib.nrc_ngp_set_encoder_block_levels(-1)
