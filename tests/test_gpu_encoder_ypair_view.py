"""The image encoder reads the hashed levels that follow the block view's dense levels through a y-pair view (include/nerficg_hip.h:
nrc_ngp_build_ypair_view -- per level a dense array of 8-byte records {fp16 pair of vertex (x, y, z), fp16 pair of vertex (x, y + 1, z)} in x + R (y + R z)
order, R = res + 2; nrc_ngp_set_encoder_ypair_view / _ypair_levels): two 16-byte loads of one address per level instead of the vertex view's four loads
or the table's hash, four loads and a predicated round of four more.  The view holds COPIES of table entries and the encoder feeds them to the same
weights in the same order, so everything here is an equality of bits: the view against a numpy restatement of the spatial hash, the feature buffer with
P = 1 .. 6 levels read through the view against P = 0, the pictures with the view against those without, a view that follows the parameters, and no view
once a recorded graph writes the table.  The feature and builder tests use a 2^14-entry grid (hashed from level 2, res 31: 19 MB for the five levels a view
holds by default, 50 MB for six); the tables
are full-range random fp16 pairs."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scenes
from tests.test_gpu_encoder_block_view import _cfg, _levels

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VIEW_LEVELS = (2, 3, 4, 5, 6, 7)      # the 2^14-entry grid: levels 0-1 dense (16^3, 23^3), res 31 43 59 81 112 154 hashed
YPAIR_MAX = 6


def _small_model():
    from nerficg_amd.instant_ngp import InstantNGPModel
    model = InstantNGPModel(RANDOM_SEED=5, HASHGRID_LOG2_SIZE=14, device=DEV)
    with torch.no_grad():
        n = model.encoding_xyz.params.numel() - 3072
        model.encoding_xyz.params[3072:] = ((torch.rand(n, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 2.0).to(DEV)
        model.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.35, 1)).to(DEV))
    return model


def _held(lib, g):
    """the levels the library's view of this grid holds (it holds what it reads by default), from its size: a prefix of the hashed levels"""
    lv = _levels(g)
    first = 0
    while first < 5 and lv[first][4] == 0:
        first += 1
    nbytes, sizes = int(lib.nrc_ngp_ypair_view_bytes(*_cfg(g))), [0]
    for l in range(first, min(first + YPAIR_MAX, len(lv))):
        sizes.append(sizes[-1] + 8 * (lv[l][2] + 2) ** 3)
    assert nbytes in sizes
    return list(range(first, first + sizes.index(nbytes))), nbytes


def test_view_holds_the_two_entries_the_hash_names():
    """record (x, y, z) of a view level is {table[hash(x, y, z)], table[hash(x, y + 1, z)]}, hash = (x ^ y 2654435761 ^ z 805459861) & (size - 1) behind the
    level's offset: every record of the first level, a seeded sample of 100 000 of each further level (the corners x, z in {0, R - 1}, y in {0, R - 2}
    among them); every record of the row y = R - 1 = res + 1 of every level is zero"""
    from nerficg_amd import _lib
    lib = _lib.load()
    g = _small_model().encoding_xyz.grid_cfg
    lv = _levels(g)
    levels, nbytes = _held(lib, g)
    assert levels and tuple(levels) == VIEW_LEVELS[:len(levels)] and [lv[l][2] for l in levels] == [31, 43, 59, 81, 112, 154][:len(levels)]
    total = lv[-1][0] + lv[-1][1]
    table = torch.from_numpy(np.random.default_rng(11).integers(1, 2 ** 32, size=total, dtype=np.uint32).view(np.int32)).to(DEV)      # (no zero entry)
    view = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.nrc_ngp_build_ypair_view(_lib.ptr(table), *_cfg(g), _lib.ptr(view), _lib.stream_of(view)), 'build')
    got = view.cpu().numpy().view(np.uint32).reshape(-1, 2)
    tab = table.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(12)
    first = 0
    for l in levels:
        off, size, res, _, _ = lv[l]
        R = res + 2
        assert size == 1 << 14
        level = got[first:first + R ** 3].reshape(R, R, R, 2)          # [z][y][x]
        assert not level[:, R - 1].any(), l
        if l == levels[0]:
            v = np.arange(R ** 3, dtype=np.int64)
        else:
            corners = np.array([x + R * (y + R * z) for x in (0, R - 1) for y in (0, R - 2) for z in (0, R - 1)], np.int64)
            v = np.concatenate([corners, rng.integers(0, R ** 3, size=100_000 - 8)])
        x, y, z = (v % R).astype(np.uint64), (v // R % R).astype(np.uint64), (v // (R * R)).astype(np.uint64)
        keep = y < R - 1
        v, x, y, z = v[keep], x[keep], y[keep], z[keep]
        h = lambda yy: ((x ^ (yy * np.uint64(2654435761)) ^ (z * np.uint64(805459861))) & np.uint64(size - 1)).astype(np.int64)
        assert np.array_equal(got[first + v, 0], tab[off + h(y)]), l
        assert np.array_equal(got[first + v, 1], tab[off + h(y + np.uint64(1))]), l
        first += R ** 3
    assert first == got.shape[0]


def _cells(lv, level, p):
    """floor(fmaf(scale, p, 0.5)) as the encoder computes it, and whether p is clear of a step of that floor"""
    f = (np.float32(lv[level][3]).astype(np.float64) * p.astype(np.float64) + 0.5).astype(np.float32)
    return np.floor(f).astype(np.int64), np.abs(f - np.round(f)) > 0.01


@pytest.fixture(scope='module')
def samples():
    """five ray tiles of 16 rows (5 120 slots) for nrc_ngp_encode_samples.  Tiles 0 and 1: ray r starts on the plane (its axis r % 3) = 0 with special
    values on the other two axes and runs along that axis with d = 1, so p = o + t d is exact and a special t puts all three coordinates on special
    values -- tile 0: cell faces, centres and their float32 neighbours at both ends and in the middle of every view level, 0, 1 and 1 - ulp; tile 1:
    centres of the cells gx = 15 (mod 16), where the 16-byte load crosses a 128-byte line, of the cells res - 1 and res (positions a little beyond 1: at
    the level they are made for the cell is still in [0, res]^3, at finer levels it is not, and those features are not compared), odd and even ones.
    Tiles 2-4: 3 072 random positions in the box."""
    from tests.test_gpu_encoder_vertex_view import _special_values
    model = _small_model()
    enc = model.encoding_xyz
    lv = _levels(enc.grid_cfg)
    tiles, rows = 5, 80
    n = rows * 64
    rng = np.random.default_rng(5)
    vals = _special_values(lv, VIEW_LEVELS)
    assert 100 < len(vals) < 1024 and vals[0] == 0.0 and vals[-1] == 1.0
    centres = []
    for l in VIEW_LEVELS:
        _, _, res, scale, _ = lv[l]
        ks = sorted(set(range(15, res, 16)) | {res - 2, res - 1, res})
        centres += [k / np.float32(scale) for k in ks]
    centres = np.asarray(centres, np.float32)
    assert len(centres) < 62 and centres.max() < 1.1
    o = np.zeros((tiles, 64, 3), np.float32)
    d = np.zeros((tiles, 64, 3), np.float32)
    ts = np.zeros((tiles, 1024), np.float32)
    axis = np.arange(64) % 3
    for t, pool in ((0, vals), (1, centres)):
        o[t] = rng.choice(np.concatenate([vals, pool]), size=(64, 3))
        if t == 0:
            for i, e in enumerate((0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)))):   # rays 3 .. 11: the two axes across the ray on an end value
                o[t, 3 + 3 * i:6 + 3 * i] = e
        o[t, np.arange(64), axis] = 0.0
        d[t, np.arange(64), axis] = 1.0
        ts[t] = rng.choice(pool, size=1024)
        ts[t, :len(pool)] = pool                                    # every value at least once ...
    for k in range(3):                                              # ... and every centre on rays of all three axes (slot s belongs to ray s % 64)
        ts[1, 64 * k + k:64 * k + k + len(centres)] = centres
    o[2:] = rng.uniform(0.1, 0.9, size=(3, 64, 3))
    d[2:] = rng.uniform(-0.1, 0.1, size=(3, 64, 3))
    ts[2:] = rng.uniform(0.0, 1.0, size=(3, 1024))
    holes = rng.random((tiles, 1024)) < 0.05
    holes[:2, :600] = False
    ts[holes] = -1.0
    ts = ts.reshape(n)
    live = ts >= 0
    assert 50 < (~live).sum()
    tile_of = np.arange(n) // 1024
    pos = o[tile_of, np.arange(n) % 64] + ts[:, None] * d[tile_of, np.arange(n) % 64]
    assert pos[live].min() >= 0.0 and pos[live & (tile_of != 1)].max() <= 1.0
    # which features are comparable (the cell of every axis in [0, res] at that level), and what the slots cover
    valid = np.ones((n, 16), bool)
    for l in VIEW_LEVELS:
        res = lv[l][2]
        for a in range(3):
            c, clear = _cells(lv, l, pos[:, a])
            valid[:, l] &= (c <= res) & (clear | (c < res))
            seen = c[live & clear & valid[:, l]]
            for want in (0, res - 1, res):
                assert (seen == want).any(), (l, a, want)
            assert (seen % 2 == 0).sum() > 10 and (seen % 2 == 1).sum() > 10 and (seen % 16 == 15).sum() > 2, (l, a)
        for a in range(3):
            assert all((pos[live, a] == e).any() for e in (np.float32(0), np.float32(1))), a
    assert valid[tile_of != 1].all() and not valid[tile_of == 1].all()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ray_od = np.concatenate([o.transpose(0, 2, 1), d.transpose(0, 2, 1)], axis=1)   # per-tile SoA [6][64]
    row_tile = (np.arange(rows) // 16).astype(np.int32)
    return enc, rows, n, T(ts), T(ray_od), T(row_tile), valid & live[:, None]


def _encode(samples, levels, view):
    """nrc_ngp_encode_samples with `levels` levels read through `view` (None: no view is set); (code, features as [slot][level] dwords)"""
    from nerficg_amd import _lib
    lib = _lib.load()
    enc, rows, n, ts_d, od_d, rt_d, _ = samples
    mn, sz = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    vp = ctypes.c_void_p
    feat = torch.full((n * 16,), 0x3C3C3C3C, dtype=torch.int32, device=DEV)
    assert lib.nrc_ngp_set_encoder_ypair_levels(levels) == 0
    if view is not None:
        assert lib.nrc_ngp_set_encoder_ypair_view(_lib.ptr(view)) == 0
    rc = lib.nrc_ngp_encode_samples(_lib.ptr(ts_d), _lib.ptr(rt_d), _lib.ptr(od_d), 0, rows, ctypes.cast(mn, vp), ctypes.cast(sz, vp),
                                    _lib.ptr(enc._table16()), *_cfg(enc.grid_cfg), _lib.ptr(feat), None, 0, _lib.stream_of(feat))
    # fragment-major: levels 4 g .. 4 g + 3 of slot j are the 16-byte vector ((j >> 5) * 4 + ((g + (j >> 5)) & 3)) * 32 + (j & 31)
    f = feat.cpu().numpy().reshape(-1, 4)
    j = np.arange(n)
    out = np.stack([f[((j >> 5) * 4 + ((g + (j >> 5)) & 3)) * 32 + (j & 31)] for g in range(4)], axis=1).reshape(n, 16)
    return rc, out


def test_features_equal_those_of_the_table_path(samples):
    """every level the view holds, P = 1 .. 6 and the default against P = 0, bit for bit, for every sample whose cell lies in [0, res]^3 at that level"""
    from nerficg_amd import _lib
    lib = _lib.load()
    enc, valid = samples[0], samples[-1]
    enc._half_params()
    view = enc._ypair_view()
    levels, nbytes = _held(lib, enc.grid_cfg)
    assert view is not None and view.numel() == nbytes and tuple(levels) == VIEW_LEVELS[:len(levels)]
    assert view.data_ptr() % 16 == 0          # a record is 8-byte aligned; a load at an odd gx is 8-byte, not 16-byte aligned
    try:
        rc, want = _encode(samples, 0, view)
        assert rc == 0
        f16 = want[valid].view(np.float16)
        assert np.isfinite(f16).all() and np.abs(f16).max() > 0.1          # features of an amplified table, not the fill pattern
        rc, none = _encode(samples, YPAIR_MAX, None)                       # no view handed over: the table, whatever is asked for
        assert rc == 0 and np.array_equal(none, want)
        for p in (1, 2, 3, 4, 5, 6, -1):
            rc, got = _encode(samples, p, view)
            assert rc == 0
            bad = (got != want) & valid
            assert not bad.any(), (p, np.argwhere(bad)[:8].tolist())
        rc, got = _encode(samples, YPAIR_MAX, torch.zeros_like(view))      # the premise: a set view is read, at exactly the levels it holds
        assert rc == 0
        differs = ((got != want) & valid).any(axis=0)
        assert differs.tolist() == [l in levels for l in range(16)]
        rc, got = _encode(samples, YPAIR_MAX, None)                        # ... and taken by the call it was set for
        assert rc == 0 and np.array_equal(got, want)
    finally:
        lib.nrc_ngp_set_encoder_ypair_levels(-1)
        lib.nrc_ngp_set_encoder_ypair_view(None)


def _pictures(renderer, cam, pose, levels=-1):
    """72 x 40 frames (partial edge tiles), single pass and slab order, with `levels` levels read through the y-pair view (-1: the default, 0: none)"""
    from nerficg_amd import _lib
    lib = _lib.load()
    out = {}
    try:
        assert lib.nrc_ngp_set_encoder_ypair_levels(levels) == 0
        for name, early in (('single pass', False), ('slab order', True)):
            r = renderer.render_image_fused(cam, pose, return_stats=True, early_termination=early)
            out[name] = {k: (r[k].clone() if torch.is_tensor(r[k]) else r[k]) for k in ('rgb', 'alpha', 'depth', 'n_samples')}
    finally:
        lib.nrc_ngp_set_encoder_ypair_levels(-1)
    return out


def _assert_same(got, want, where):
    for name in want:
        for k, v in want[name].items():
            assert (torch.equal(got[name][k], v) if torch.is_tensor(v) else got[name][k] == v), (where, name, k)


def test_frames_with_the_view_equal_frames_without_and_follow_the_parameters():
    """the shipped grid (view of levels 5 and up): rgb, alpha, depth and n_samples with P = 1 .. 6 and the default are those with P = 0 (the vertex view or
    the table at those levels); the renderer allocates no vertex view where the y-pair view holds its levels; after an optimizer step the view is rebuilt
    and the pictures are again the table path's, and not the ones before"""
    from nerficg_amd import _lib
    from nerficg_amd.apex_optimizers import FusedAdam
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    lib = _lib.load()
    model = make_model()
    enc = model.encoding_xyz
    cam, pose = make_camera(72, 40, bg=(0.2, 0.4, 0.6)), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    renderer = InstantNGPRenderer(model)
    first = _pictures(renderer, cam, pose)
    levels, nbytes = _held(lib, enc.grid_cfg)
    view = enc._ypair_view()
    assert float(first['single pass']['alpha'].max()) > 0.1 and first['single pass']['n_samples'] > 0
    if levels:
        assert view is not None and view.numel() == nbytes and enc._ypair_view() is view       # valid from frame to frame
        assert (enc._vview is None) == (len(levels) >= 4)                                      # levels 5-8 are the vertex view's
    else:
        assert view is None and enc._vview is not None
    want = _pictures(renderer, cam, pose, levels=0)
    _assert_same(first, want, 'default')
    for p in range(1, YPAIR_MAX + 1):
        _assert_same(_pictures(renderer, cam, pose, levels=p), want, p)
    opt = FusedAdam(model.parameters(), lr=1e-1, eps=1e-15, betas=(0.9, 0.99), adam_w_mode=False)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    second = _pictures(renderer, cam, pose)
    _assert_same(second, _pictures(renderer, cam, pose, levels=0), 'optimizer step')
    assert not torch.equal(second['single pass']['rgb'], first['single pass']['rgb'])


def test_frames_after_a_replayed_optimiser_step_have_no_view():
    """A HIP-graph replay rewrites the fp16 table with no Python in between.  From the recording on, the module has no y-pair view (and has freed it): render,
    replays, render -- the second picture is the table path's on the trained model, and not the first."""
    from nerficg_amd.apex_optimizers import FusedAdam
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    model = make_model()
    enc = model.encoding_xyz
    renderer = InstantNGPRenderer(model)
    cam, pose = make_camera(72, 40), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15, betas=(0.9, 0.99), adam_w_mode=False, capturable=True)
    for p in model.parameters():       # a fixed gradient: every entry moves by about lr per step
        p.grad = torch.ones_like(p)
    opt.step()                         # eager: creates the moments
    first = _pictures(renderer, cam, pose)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    before = enc.params.detach().clone()
    for _ in range(3):
        graph.replay()
    assert not torch.equal(enc.params.detach()[3072:], before[3072:])     # the replays trained the table
    second = _pictures(renderer, cam, pose)
    assert enc._ypair_view() is None and enc._yview is None
    _assert_same(second, _pictures(renderer, cam, pose, levels=0), 'replayed')
    assert torch.equal(enc._half_params(), enc.params.detach().half())   # the copy the table path read is current
    assert not torch.equal(second['single pass']['rgb'], first['single pass']['rgb'])
