"""The single-pass frame has three forms (nrc_ngp_set_frame_density_encoder, nrc_ngp_set_frame_full_encoder; InstantNGPRenderer.FRAME_DENSITY_ENCODER,
FRAME_FULL_ENCODER):

  full   k_grid_encode<SRC_TILED, true, true> runs the density net AND the colour net on the 64 samples of its own wave and stores the 8-byte record
         (h0, r, g, b) of every sample at its absolute slot; one launch of k_composite_image composites them;
  32 B   FRAME_FULL_ENCODER = 0: the density-encoder pair, k_ngp_mlp_composite<true> runs the colour net and composites;
  64 B   FRAME_DENSITY_ENCODER = 0: the encoder writes grid features, k_ngp_mlp_composite<false> runs both nets (whatever FRAME_FULL_ENCODER says).

The three run the same MFMAs on the same operands and the same per-sample compositing step, so they must paint THE SAME BITS: rgb, alpha, depth and the
sample count of render_image_fused(early_termination=False) are compared with torch.equal, no tolerance.  The model's table is U(-2, 2) and its density
AND colour weights are N(0, 0.5): no output is degenerate, and the SH operand of the colour net matters.  The workspace is filled with 0xA5 in front of
every compared frame, so that a record nobody wrote, or one written to the wrong place, shows in the picture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import colour_frag_image_ref as cref
from tests import scenes

DEV = 'cuda'
KEYS = ('rgb', 'alpha', 'depth')
pytestmark = pytest.mark.gpu
POSE = scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)
FORMS = {'full': (1, 1), '32 B': (1, 0), '64 B': (0, 1)}   # name -> (FRAME_DENSITY_ENCODER, FRAME_FULL_ENCODER)


@pytest.fixture(scope='module')
def lib():
    from nerficg_amd import _lib
    return _lib.load()


def _set_weights(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.encoding_xyz.params[:3072] = (torch.randn(3072, generator=g) * 0.5).to(DEV)
        m.color_mlp_with_encoding.params[:] = (torch.randn(m.color_mlp_with_encoding.params.numel(), generator=g) * 0.5).to(DEV)


def _set_colour_weights(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.color_mlp_with_encoding.params[:] = (torch.randn(m.color_mlp_with_encoding.params.numel(), generator=g) * 0.5).to(DEV)


def _model(radius=0.35):
    """the seeded model of the frame tests (table entries U(-2, 2)) with density and colour weights N(0, 0.5) and a ball as occupancy"""
    from tests.test_gpu_render_parity import make_model
    m = make_model()
    _set_weights(m, 21)
    with torch.no_grad():
        if radius > 0:
            m.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, radius, 1)).to(DEV))
        else:
            m.occupancy_bitfield.zero_()
    return m


@pytest.fixture(scope='module')
def model():
    return _model()


@pytest.fixture(autouse=True)
def _settings_back(lib):
    yield
    lib.nrc_ngp_set_frame_density_encoder(-1)
    lib.nrc_ngp_set_frame_full_encoder(-1)
    lib.nrc_ngp_set_encoder_shape(-1, -1)
    lib.nrc_ngp_set_encoder_block_levels(-1)
    lib.nrc_ngp_set_encoder_vertex_levels(-1)
    lib.nrc_ngp_set_encoder_ypair_levels(-1)


def _form(renderer, name):
    renderer.FRAME_DENSITY_ENCODER, renderer.FRAME_FULL_ENCODER = FORMS[name]


def _fill(renderer, name):
    for ws in renderer._fused_ws.values():
        if ws.get('fws') is not None:
            assert ws['fws_key'][2:] == FORMS[name]
            ws['fws'].fill_(0xA5)


def _copy(res):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}


def _same(a, b, what=''):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (k, what)
    for k in ('n_rows', 'n_samples'):
        assert a[k] == b[k], (k, what)


def _stages(frame):
    """the stage labels of one frame() (the library's stage timer): which kernels the frame launched"""
    from nerficg_amd import _lib
    with _lib.stage_timer() as st:
        frame()
        torch.cuda.synchronize()
    return set(st.by_name())


def _all_forms(renderer, frame, full_runs=True):
    """frame() under the three forms, the workspace overwritten in front of each compared frame -> the result of the 64-byte pair.  The first frame of every
    form says through its stage labels which kernels ran: the full form (where full_runs: the frame is within eight row budgets) composites in
    "k_composite_image" and has no "k_ngp_mlp" / "k_tile_chunks" stage, the pairs -- and the full setting's fallback -- the reverse"""
    got = {}
    for name in FORMS:
        _form(renderer, name)
        labels = _stages(frame)   # (allocates the workspace)
        if full_runs is None:   # (a frame without rows: the renderer does not call nrc_ngp_render_frame at all)
            pass
        elif name == 'full' and full_runs:
            assert 'k_composite_image' in labels and not labels & {'k_ngp_mlp', 'k_tile_chunks'}, labels
        else:
            assert {'k_ngp_mlp', 'k_tile_chunks'} <= labels and 'k_composite_image' not in labels, (name, labels)
        _fill(renderer, name)
        got[name] = _copy(frame())
    _same(got['64 B'], got['full'], 'full')
    _same(got['64 B'], got['32 B'], '32 B')
    return got['64 B']


def _image(renderer, cam, pose=POSE, **kw):
    return lambda: renderer.render_image_fused(cam, pose, early_termination=False, return_stats=True, **kw)


def _varies(out):
    a, c = out['alpha'], out['rgb']
    assert float(a.max()) > 0.1 and float(a.max()) > float(a.min()), 'alpha is constant over the picture'
    spread = c.max(dim=0).values - c.min(dim=0).values   # (sanity of the scene, not a tolerance: the forms are compared bit for bit)
    assert float(spread.min()) > 0.0 and float(spread.max()) > 0.1, 'a colour channel is constant over the picture'


@pytest.mark.parametrize('size', [(40, 24), (20, 12)])
def test_small_ball(model, size):
    """partial tiles on both edges (slots behind n in the last block of 1024), holes in every row of a tile's tail"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    out = _all_forms(r, _image(r, make_camera(*size, bg=(0.2, 0.4, 0.6))))
    assert out['n_rows'] > 16 and 0 < out['n_samples'] < out['n_rows'] * 64
    _varies(out)


def test_empty_grid():
    """no rows at all: no encoder launch under any setting, the compositor paints the background"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(_model(radius=0.0))
    out = _all_forms(r, _image(r, make_camera(40, 24, bg=(0.25, 0.5, 1.0))), full_runs=None)
    assert out['n_rows'] == 0 and out['n_samples'] == 0 and float(out['alpha'].max()) == 0.0


@pytest.mark.parametrize('shape', [(3, 1), (2, 2), (2, 1)])   # 8 x 2 x 4, 4 x 4 x 4, 4 x 2 x 8
def test_every_encoder_shape(model, lib, shape):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    r.POSE_ENCODER_SHAPE = False   # the shape set here, not the pose's
    assert lib.nrc_ngp_set_encoder_shape(*shape) == 0
    _varies(_all_forms(r, _image(r, make_camera(40, 24))))


def test_several_chunks(model):
    """FRAME_ROW_BUDGET = 2048: the pairs run >= 3 rounds of whole ray tiles; the full form stores every record at its absolute slot (n_rows <= 8 budgets)"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    r.FRAME_ROW_BUDGET = 2048
    out = _all_forms(r, _image(r, make_camera(48, 32)))
    assert 8 * 2048 >= out['n_rows'] > 2048 and -(-out['n_rows'] // (2048 - r.MAX_SAMPLES)) >= 3
    one = InstantNGPRenderer(model)
    _same(out, _copy(_image(one, make_camera(48, 32))()), 'one chunk, the default form')
    _varies(out)


def test_more_rows_than_eight_budgets(model):
    """n_rows > 8 x the row budget: the records of the full form would not fit the feature part, the frame falls back to the 32-byte pair -- same bits"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model, MAX_SAMPLES=256)
    r.FRAME_ROW_BUDGET = 512
    out = _all_forms(r, _image(r, make_camera(96, 64)), full_runs=False)
    assert out['n_rows'] > 8 * 512
    _varies(out)


def test_cascades_and_exponential_steps():
    """SCALE = 2 (three cascades, a box that is not the unit box: the division in fetch_pos) with exponential steps"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_garden_parity import garden_camera, garden_model
    m = garden_model()
    assert m.cascades == 3 and float(m.SCALE) == 2.0
    _set_weights(m, 22)
    r = InstantNGPRenderer(m, EXPONENTIAL_STEPS=True)
    out = _all_forms(r, _image(r, garden_camera(40, 24), scenes.orbit_pose(0.4, 0.15, 1.15)))
    assert out['n_samples'] > 0 and float(out['alpha'].max()) > 0.1


@pytest.mark.parametrize('views', [True, False])
def test_with_the_three_views_and_with_none(model, lib, views):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    levels = -1 if views else 0
    assert lib.nrc_ngp_set_encoder_block_levels(levels) == 0 and lib.nrc_ngp_set_encoder_vertex_levels(levels) == 0
    assert lib.nrc_ngp_set_encoder_ypair_levels(levels) == 0
    r = InstantNGPRenderer(model)
    _varies(_all_forms(r, _image(r, make_camera(40, 24))))


def test_a_tile_shard(model):
    """tile_begin > 0: the compositor's pixel addresses start behind tile 0, the records' slots at 0"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    cam = make_camera(40, 24, bg=(0.2, 0.4, 0.6))
    n_tiles = 5 * 3
    r = InstantNGPRenderer(model)
    out = _all_forms(r, _image(r, cam, tile_begin=n_tiles // 3, n_tiles=n_tiles // 2))
    assert out['n_samples'] > 0


def test_the_ray_list_door(model):
    """render_rays_fused with 100 rays: two tiles, the second one with 36 rays"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from nerficg_amd.raygen import generate_rays
    from tests.test_gpu_render_parity import make_camera
    cam = make_camera(20, 12)
    rays = generate_rays(cam.width, cam.height, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, POSE, want_direction=False)
    origin, direction = rays['origin'][70:170].contiguous(), rays['view_direction'][70:170].contiguous()
    r = InstantNGPRenderer(model)
    out = _all_forms(r, lambda: r.render_rays_fused(origin, direction, cam, early_termination=False, return_stats=True))
    assert out['rgb'].shape == (100, 3) and out['n_samples'] > 0
    _varies(out)


def test_colour_weights_changed_between_two_frames():
    """the same renderer, the same workspace: the frame behind a change of the colour weights follows the new weights (the image is rebuilt by every frame)
    -- first with the workspace as the earlier frame left it, then overwritten"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    m = _model()
    cam = make_camera(40, 24, bg=(0.2, 0.4, 0.6))
    r = InstantNGPRenderer(m)
    _form(r, 'full')
    frame = _image(r, cam)
    first = _copy(frame())
    _set_colour_weights(m, 23)
    second = _copy(frame())          # (the workspace still holds the first frame's image)
    _fill(r, 'full')
    third = _copy(frame())
    assert not torch.equal(first['rgb'], second['rgb']) and torch.equal(first['alpha'], second['alpha'])
    _same(second, third)
    r0 = InstantNGPRenderer(m)
    _form(r0, '64 B')
    _same(_copy(_image(r0, cam)()), second)
    _varies(second)


def test_exact_workspace_and_guard(model, lib):
    """a frame rendered into a workspace of exactly nrc_ngp_render_frame_ws_bytes, its feature part filled with 0xA5 (as everything else), leaves the 4 KB
    behind it untouched, ends with the colour image and the density image, and paints what the renderer's own workspace paints"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests import density_frag_image_ref as dref
    from tests.test_gpu_render_parity import make_camera
    cam = make_camera(40, 24, bg=(0.2, 0.4, 0.6))
    for budget in (0, 2048):
        r = InstantNGPRenderer(model)
        _form(r, 'full')
        if budget:
            r.FRAME_ROW_BUDGET = budget
        want = _copy(_image(r, cam)())
        held = []
        entry = r._frame_entry

        def exact(fn, args, what, views):
            if what == 'ngp_render_frame':
                assert len(args) == 31
                n = int(lib.nrc_ngp_render_frame_ws_bytes(args[3], args[4], args[22], args[28]))
                buf = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
                held.append((buf, n))
                args = list(args)
                args[29] = ctypes.c_void_p(buf.data_ptr())
            return entry(fn, args, what, views)

        r._frame_entry = exact
        got = _copy(_image(r, cam)())
        torch.cuda.synchronize()
        assert len(held) == 1
        buf, n = held[0]
        assert bool((buf[n:] == 0xA5).all()), budget
        wd = model.encoding_xyz._half_params()[:3072].cpu().numpy()
        wc = model.color_mlp_with_encoding._half_params().cpu().numpy()
        assert np.array_equal(buf[n - 6144:n].cpu().numpy(), np.frombuffer(dref.image_of(wd).tobytes(), np.uint8)), budget
        assert np.array_equal(buf[n - 6144 - 14336:n - 6144].cpu().numpy(), np.frombuffer(cref.image_of(wc).tobytes(), np.uint8)), budget
        _same(want, got)


def test_the_setter_and_the_workspace(lib):
    """-1, 0, 1 and nothing else; the workspace has one size whichever form is set"""
    assert [lib.nrc_ngp_set_frame_full_encoder(v) for v in (-2, 2)] == [-1, -1]
    rows, tiles = 4096, 100
    for budget, feat_rows in ((0, 4096), (2048, 2048)):   # one chunk; several
        sizes = set()
        for dens in (-1, 0, 1):
            for full in (-1, 0, 1):
                assert lib.nrc_ngp_set_frame_density_encoder(dens) == 0 and lib.nrc_ngp_set_frame_full_encoder(full) == 0
                sizes.add(int(lib.nrc_ngp_render_frame_ws_bytes(rows, tiles, 1024, budget)))
        assert len(sizes) == 1 and sizes.pop() >= feat_rows * 64 * 64 + 6144 + 14336
