"""GPU: the density net's fragment image (C ABI group 29) and the frames that read it.

nrc_ngp_render_frame writes the density net's six MFMA A fragments into the tail of its workspace in every call, and the density-encoder form of
k_grid_encode copies them into LDS instead of building them from the row-major weights.  The fragments hold the same fp16 values on the same lanes, so
  * the image nrc_ngp_density_frag_image writes is BYTE-equal to the numpy restatement (tests/density_frag_image_ref.py), and
  * the density-encoder pair (nrc_ngp_set_frame_density_encoder(1)) paints the same BITS as the 64-byte pair (0), which never reads the image:
    rgb, alpha, depth and the sample count are compared with torch.equal, no tolerance.
The model is built so that a misplaced weight cannot hide: table entries of order 1 and density weights N(0, 0.5) -- every frame test asserts that alpha
varies over the picture.  The workspace is filled with 0x3C in front of every compared frame: an image nobody wrote shows in the picture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import density_frag_image_ref as ref
from tests import scenes

DEV = 'cuda'
KEYS = ('rgb', 'alpha', 'depth')
pytestmark = pytest.mark.gpu
POSE = scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS)


@pytest.fixture(scope='module')
def lib():
    from nerficg_amd import _lib
    return _lib.load()


def _set_density_weights(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.encoding_xyz.params[:3072] = (torch.randn(3072, generator=g) * 0.5).to(DEV)


def _model(radius=0.35):
    """the seeded model of the frame tests (table entries U(-2, 2)) with density weights N(0, 0.5) and a ball as occupancy"""
    from tests.test_gpu_render_parity import make_model
    m = make_model()
    _set_density_weights(m, 11)
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


def _fill(renderer, mode):
    for ws in renderer._fused_ws.values():
        if ws.get('fws') is not None:
            assert ws['fws_key'][2] == mode
            ws['fws'].fill_(0x3C)


def _copy(res):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}


def _same(a, b):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    for k in ('n_rows', 'n_samples'):
        assert a[k] == b[k], k


def _both_pairs(renderer, frame):
    """frame() under pair 0 and under pair 1, the workspace overwritten in front of each compared frame -> the result of pair 0"""
    got = {}
    for mode in (0, 1):
        renderer.FRAME_DENSITY_ENCODER = mode
        frame()   # (allocates the workspace)
        _fill(renderer, mode)
        got[mode] = _copy(frame())
    _same(got[0], got[1])
    return got[0]


def _image(renderer, cam, pose=POSE):
    return lambda: renderer.render_image_fused(cam, pose, early_termination=False, return_stats=True)


def _varies(out):
    a = out['alpha']
    assert float(a.max()) > 0.1 and float(a.max()) > float(a.min()), 'alpha is constant over the picture'


def test_image_content(lib):
    """all 3 072 halves distinct: every byte of the 6 KB says which weight it came from"""
    from nerficg_amd import _lib
    w = ref.distinct_weights()
    wd = torch.from_numpy(w).to(DEV)
    out = torch.full((6144 + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nrc_ngp_density_frag_image(_lib.ptr(wd), _lib.ptr(out), _lib.stream_of(wd)), 'ngp_density_frag_image')
    got = out.cpu().numpy()
    want = ref.image_of(w)
    assert want.nbytes == 6144
    assert np.array_equal(got[:6144], np.frombuffer(want.tobytes(), np.uint8))
    assert (got[6144:] == 0xA5).all()   # nothing behind the image
    assert lib.nrc_ngp_density_frag_image(None, _lib.ptr(out), _lib.stream_of(wd)) == -1
    assert lib.nrc_ngp_density_frag_image(_lib.ptr(wd), None, _lib.stream_of(wd)) == -1


@pytest.mark.parametrize('size', [(40, 24), (20, 12)])
def test_small_ball(model, size):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    out = _both_pairs(r, _image(r, make_camera(*size, bg=(0.2, 0.4, 0.6))))
    assert out['n_rows'] > 16 and out['n_samples'] > 0
    _varies(out)


def test_empty_grid():
    """no rows at all: the encoder is not launched, the extra workgroup of the first launch still runs"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(_model(radius=0.0))
    out = _both_pairs(r, _image(r, make_camera(40, 24, bg=(0.25, 0.5, 1.0))))
    assert out['n_rows'] == 0 and out['n_samples'] == 0 and float(out['alpha'].max()) == 0.0


def test_several_chunks(model):
    """a row budget of two tiles' capacity: >= 3 rounds; the image sits behind a chunk table of several entries"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    r = InstantNGPRenderer(model)
    r.FRAME_ROW_BUDGET = 2 * r.MAX_SAMPLES
    out = _both_pairs(r, _image(r, make_camera(48, 32)))
    assert out['n_rows'] > r.FRAME_ROW_BUDGET and -(-out['n_rows'] // (r.FRAME_ROW_BUDGET - r.MAX_SAMPLES)) >= 3
    _varies(out)


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
    assert out['rgb'].shape == (100, 3) and out['n_samples'] > 0
    _varies(out)


def test_weights_changed_between_two_frames():
    """the same renderer, the same workspace: the frame behind a change of the density weights follows the new weights (the image is rebuilt by every
    frame, nothing is kept from the frame before) -- first with the workspace as the earlier frame left it, then overwritten"""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    m = _model()
    cam = make_camera(40, 24, bg=(0.2, 0.4, 0.6))
    r = InstantNGPRenderer(m)
    r.FRAME_DENSITY_ENCODER = 1
    frame = _image(r, cam)
    first = _copy(frame())
    _set_density_weights(m, 12)
    second = _copy(frame())          # (the workspace still holds the first frame's image)
    _fill(r, 1)
    third = _copy(frame())
    assert not torch.equal(first['alpha'], second['alpha'])
    _same(second, third)
    r0 = InstantNGPRenderer(m)
    r0.FRAME_DENSITY_ENCODER = 0
    want = _copy(_image(r0, cam)())
    _same(want, second)
    _varies(second)


def test_workspace_size_and_guard(model, lib):
    """one size for both pairs, at least 64 B per slot; a frame rendered into a workspace of exactly nrc_ngp_render_frame_ws_bytes leaves the 4 KB
    behind it untouched and paints what the renderer's own (larger) workspace paints"""
    from nerficg_amd import _lib
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera
    rows, tiles = 4096, 100
    assert lib.nrc_ngp_set_frame_density_encoder(0) == 0
    b0 = lib.nrc_ngp_render_frame_ws_bytes(rows, tiles, 1024, 0)
    assert lib.nrc_ngp_set_frame_density_encoder(1) == 0
    b1 = lib.nrc_ngp_render_frame_ws_bytes(rows, tiles, 1024, 0)
    assert b0 == b1 and b0 >= rows * 64 * 64 + 6144
    cam = make_camera(40, 24, bg=(0.2, 0.4, 0.6))
    for budget in (0, 2048):   # one chunk; several
        for mode in (0, 1):
            r = InstantNGPRenderer(model)
            r.FRAME_DENSITY_ENCODER = mode
            if budget:
                r.FRAME_ROW_BUDGET = budget
            want = _copy(_image(r, cam)())
            held = []
            entry = r._frame_entry

            def exact(fn, args, what, views):
                if what == 'ngp_render_frame':
                    assert len(args) == 31
                    n = int(lib.nrc_ngp_render_frame_ws_bytes(args[3], args[4], args[22], args[28]))
                    assert n >= (min(args[3], budget) if budget else args[3]) * 64 * 64   # (64 B per slot of the largest chunk)
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
            assert bool((buf[n:] == 0xA5).all()), (budget, mode)
            tail = buf[n - 6144:n].cpu().numpy()   # 6 144 is a multiple of 256: the image is the last thing in the workspace
            wd = model.encoding_xyz._half_params()[:3072].cpu().numpy()
            assert np.array_equal(tail, np.frombuffer(ref.image_of(wd).tobytes(), np.uint8)), (budget, mode)
            _same(want, got)
