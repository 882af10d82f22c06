"""The single-pass frame has two kernel pairs (nrc_ngp_set_frame_density_encoder; InstantNGPRenderer.FRAME_DENSITY_ENCODER):

  0  k_grid_encode writes the 64 B of grid features of every slot, k_ngp_mlp_composite runs the density net, its head and the colour net;
  1  k_grid_encode<SRC_TILED, true> runs the density net on the 64 samples of its own wave (two MFMA tiles, whatever slots its brick holds) and writes
     the 16 fp16 density features, 32 B per slot; k_ngp_mlp_composite<true> runs the colour net from there.

The existing suite holds pair 0 against float64 (tests/test_gpu_frame_stages.py and the parity tests).  Pair 1 runs the same MFMAs on the same operands
-- a sample's column in a tile differs, and the columns of an MFMA are independent -- so it must paint THE SAME BITS: rgb, alpha, depth and the sample
count of render_image_fused(early_termination=False) are compared with torch.equal, no tolerance.  The feature workspace is filled with fp16 1.06
in front of every compared frame, so that a record nobody wrote, or one written to the wrong place, shows in the picture."""
import numpy as np
import pytest
import torch

from tests import scenes

DEV = 'cuda'
KEYS = ('rgb', 'alpha', 'depth')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from nerficg_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def model():
    """the seeded model of the frame tests (full-range table), sphere occupancy of radius 0.35"""
    from tests.test_gpu_render_parity import make_model
    m = make_model()
    with torch.no_grad():
        m.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.35, 1)).to(DEV))
    return m


@pytest.fixture(autouse=True)
def _settings_back(lib):
    yield
    lib.nrc_ngp_set_frame_density_encoder(-1)
    lib.nrc_ngp_set_encoder_shape(-1, -1)
    lib.nrc_ngp_set_encoder_block_levels(-1)
    lib.nrc_ngp_set_encoder_vertex_levels(-1)
    lib.nrc_ngp_set_encoder_ypair_levels(-1)


def _both_pairs(renderer, frame):
    """frame() with the setter at 0 and at 1 -> the two results (copies), compared bit for bit; returns the result of pair 0"""
    got = {}
    for mode in (0, 1):
        renderer.FRAME_DENSITY_ENCODER = mode
        frame()   # (allocates the workspace)
        for ws in renderer._fused_ws.values():
            if ws.get('fws') is not None:
                assert ws['fws_key'][2] == mode
                ws['fws'].fill_(0x3C)
        res = frame()
        got[mode] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}
    for k in KEYS:
        assert torch.equal(got[0][k], got[1][k]), k
    for k in ('n_rows', 'n_samples'):
        assert got[0][k] == got[1][k], k
    return got[0]


def _image(renderer, cam, pose):
    return lambda: renderer.render_image_fused(cam, pose, early_termination=False, return_stats=True)


POSE = scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)


@pytest.mark.parametrize('size', [(40, 24), (20, 12)])
def test_small_frames(model, size):
    """partial tiles on both edges; the tiles' row counts are no multiples of 16, so a block of 1024 slots spans two ray tiles and a brick holds rows of both"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    out = _both_pairs(r, _image(r, make_camera(*size, bg=(0.2, 0.4, 0.6)), POSE))
    assert out['n_rows'] > 16 and out['n_samples'] > 0
    assert float(out['alpha'].max()) > 0.1 and float(out['alpha'].min()) == 0.0   # a picture with a background around it


@pytest.mark.parametrize('shape', [(3, 1), (2, 2), (2, 1)])   # 8 x 2 x 4, 4 x 4 x 4, 4 x 2 x 8
def test_every_encoder_shape(model, lib, shape):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    r.POSE_ENCODER_SHAPE = False   # the shape set here, not the pose's
    assert lib.nrc_ngp_set_encoder_shape(*shape) == 0
    out = _both_pairs(r, _image(r, make_camera(40, 24), POSE))
    assert out['n_samples'] > 0 and float(out['alpha'].max()) > 0.1


def test_empty_frames(lib):
    """an empty occupancy grid (no rows at all: the encoder is not launched) and a small ball (most ray tiles have no rows)"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    m = make_model()
    cam = make_camera(40, 24, bg=(0.25, 0.5, 1.0))
    with torch.no_grad():
        m.occupancy_bitfield.zero_()
    r = InstantNGPRenderer(m)
    out = _both_pairs(r, _image(r, cam, POSE))
    assert out['n_rows'] == 0 and out['n_samples'] == 0 and float(out['alpha'].max()) == 0.0
    with torch.no_grad():
        m.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.1, 1)).to(DEV))
    r = InstantNGPRenderer(m)
    out = _both_pairs(r, _image(r, cam, POSE))
    covered = (out['alpha'].reshape(24, 40) > 0).cpu().numpy()
    tiles = [covered[y:y + 8, x:x + 8].any() for y in range(0, 24, 8) for x in range(0, 40, 8)]
    assert out['n_samples'] > 0 and any(tiles) and not all(tiles)


def test_several_chunks(model):
    """a row budget of two tiles' capacity: the frame runs in >= 3 rounds of whole ray tiles, each with its own records at the start of the workspace"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    r.FRAME_ROW_BUDGET = 2 * r.MAX_SAMPLES
    out = _both_pairs(r, _image(r, make_camera(48, 32), POSE))
    assert out['n_rows'] > r.FRAME_ROW_BUDGET and -(-out['n_rows'] // (r.FRAME_ROW_BUDGET - r.MAX_SAMPLES)) >= 3
    one = InstantNGPRenderer(model)
    one.FRAME_DENSITY_ENCODER = 1
    whole = one.render_image_fused(make_camera(48, 32), POSE, early_termination=False)
    for k in KEYS:
        assert torch.equal(whole[k], out[k]), k


def test_cascades_and_exponential_steps():
    """SCALE = 2 (three cascades, a box that is not the unit box: the division in fetch_pos) with exponential steps"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_garden_parity import garden_camera, garden_model
    m = garden_model()
    assert m.cascades == 3 and float(m.SCALE) == 2.0
    r = InstantNGPRenderer(m, EXPONENTIAL_STEPS=True)
    out = _both_pairs(r, _image(r, garden_camera(40, 24), scenes.orbit_pose(0.4, 0.15, 1.15)))
    assert out['n_samples'] > 0 and float(out['alpha'].max()) > 0.1


@pytest.mark.parametrize('views', [True, False])
def test_with_the_three_views_and_with_none(model, lib, views):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    levels = -1 if views else 0
    assert lib.nrc_ngp_set_encoder_block_levels(levels) == 0 and lib.nrc_ngp_set_encoder_vertex_levels(levels) == 0
    assert lib.nrc_ngp_set_encoder_ypair_levels(levels) == 0
    r = InstantNGPRenderer(model)
    out = _both_pairs(r, _image(r, make_camera(40, 24), POSE))
    assert out['n_samples'] > 0 and float(out['alpha'].max()) > 0.1


def test_the_ray_list_door(model):
    """render_rays_fused with 100 rays: two tiles, the second one with 36 rays"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from nerficg_amd.raygen import generate_rays
    from tests.test_gpu_render_parity import make_camera
    cam = make_camera(20, 12)
    rays = generate_rays(cam.width, cam.height, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, POSE, want_direction=False)
    origin, direction = rays['origin'][70:170].contiguous(), rays['view_direction'][70:170].contiguous()
    r = InstantNGPRenderer(model)
    out = _both_pairs(r, lambda: r.render_rays_fused(origin, direction, cam, early_termination=False, return_stats=True))
    assert out['rgb'].shape == (100, 3) and out['n_samples'] > 0 and float(out['alpha'].max()) > 0.1


def test_the_setter_and_the_workspace(lib):
    """-1, 0, 1 and nothing else; the workspace has one size, that of the 64-byte pair, whichever pair is set: a caller that sized it once may switch"""
    try:
        assert [lib.nrc_ngp_set_frame_density_encoder(v) for v in (-2, 2, 7)] == [-1, -1, -1]
        rows, tiles = 4096, 100
        assert lib.nrc_ngp_set_frame_density_encoder(0) == 0
        b0 = lib.nrc_ngp_render_frame_ws_bytes(rows, tiles, 1024, 0)
        assert lib.nrc_ngp_set_frame_density_encoder(1) == 0
        b1 = lib.nrc_ngp_render_frame_ws_bytes(rows, tiles, 1024, 0)
        assert b0 == b1 and b0 >= rows * 64 * 64
        assert lib.nrc_ngp_set_frame_density_encoder(-1) == 0
        assert lib.nrc_ngp_render_frame_ws_bytes(rows, tiles, 1024, 0) == b0
    finally:
        lib.nrc_ngp_set_frame_density_encoder(-1)
