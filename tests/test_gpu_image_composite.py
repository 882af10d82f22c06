"""GPU: the image compositor against the float64 reference of tests/image_composite_ref.py, every pixel of rgb, alpha and depth judged by
its own f32 budget (threshold rays by their widened one).

  a. nrc_ngp_composite_image alone, through the C ABI with raw pointers, on the synthetic tiled frames: per-lane counts of 0 .. 70 in one
     tile, early stops at different samples, all three step regimes with the `cascades` upper clamp, h0 from -inf to +89, colours outside
     [0, 1], shards, the arena form of `ts`, a row capacity that cuts a tile short.
  b. whole frames, separated from the networks: a frame rendered with compact rows leaves its fp16 network outputs, positions, counts and
     offsets in the renderer's workspace; those are composited by the reference and compared with that frame's picture, with the default
     single-pass frame (compositing inside the MLP kernel) and with the slab-order frame.  The three are bit-identical to each other by
     construction (tests/test_gpu_frame_composite.py, test_gpu_render_parity.py); here they get an absolute anchor at ~1e-6 instead of 2e-3.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import image_composite_ref as ic
from tests import scenes

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _composite(case, fill=-7.0):
    """nrc_ngp_composite_image on a case's arrays; the image buffers are pre-filled with `fill`.  Returns numpy (H*W, 3), (H*W), (H*W)."""
    from nerficg_amd import _lib
    lib = _lib.load()
    T = lambda a: torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cases are read-only)
    packed, ts, cnt, off = T(case['packed'].view(np.int16)), T(case['ts']), T(case['ray_cnt']), T(case['tile_off'])
    hw = case['width'] * case['height']
    rgb, alpha, depth = (torch.full(s, fill, device=DEV) for s in ((hw, 3), (hw,), (hw,)))
    bg = (ctypes.c_float * 3)(*[float(v) for v in case['bg3']])
    _lib.check(lib.nrc_ngp_composite_image(
        _lib.ptr(packed), _lib.ptr(ts), _lib.ptr(cnt), _lib.ptr(off), case['width'], case['height'], case['tile_begin'], case['n_tiles'], case['cascades'],
        float(case['esf']), case['grid_size'], case['max_samples'], float(case['T_threshold']), ctypes.cast(bg, ctypes.c_void_p), _lib.ptr(rgb), _lib.ptr(alpha),
        _lib.ptr(depth), case['row_capacity'], case['arena_rows'], _lib.stream_of(rgb)), 'ngp_composite_image')
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), alpha.cpu().numpy(), depth.cpu().numpy()


def _judge(pictures, ref, name):
    rgb, alpha, depth = pictures
    pix = ref['pix']
    worst = ic.assert_pixels_within_budget(dict(rgb=rgb[pix], alpha=alpha[pix], depth=depth[pix]), ref, name)
    print(f'\n{name}: err / budget {worst}')
    return worst


@pytest.mark.parametrize('name', tuple(ic.cases()))
def test_composite_image_on_the_synthetic_frames(name):
    case, ref = ic.cases()[name], ic.reference(name)
    rgb, alpha, depth = _composite(case)
    _judge((rgb, alpha, depth), ref, name)
    # pixels outside the shard keep what they held; outside the image there is nothing to write to (the buffers have H * W entries)
    rest = np.ones(case['width'] * case['height'], bool)
    rest[ref['pix']] = False
    assert rest.any() == (case['n_tiles'] < ic.N_TILES)
    assert (rgb[rest] == -7).all() and (alpha[rest] == -7).all() and (depth[rest] == -7).all()
    # rays without samples: the background, exactly
    none = ref['n'][ref['inside']] == 0
    bg = np.clip(np.asarray(case['bg3'], np.float32), 0, 1)
    p = ref['pix'][none]
    assert none.any() and (alpha[p] == 0).all() and (depth[p] == 0).all() and (rgb[p] == bg).all()


def test_the_arena_form_and_the_capacity_cut_are_bit_exact_restatements():
    plain = _composite(ic.cases()['plain'])
    arena = _composite(ic.cases()['arena'])
    for a, b in zip(plain, arena):
        np.testing.assert_array_equal(a, b)
    # row_capacity in the middle of tile 3 = the same frame with the counts cut by hand (tiles before it whole, tile 3 cut, later tiles empty)
    case = ic.cases()['capacity']
    off = case['tile_off'].astype(np.int64)
    tile = np.repeat(np.arange(ic.N_TILES), 64)
    cut = dict(ic.cases()['plain'])
    cut['ray_cnt'] = np.where(tile == 3, np.minimum(case['ray_cnt'], case['row_capacity'] - off[3]), np.where(tile > 3, 0, case['ray_cnt'])).astype(np.int32)
    for a, b in zip(_composite(case), _composite(cut)):
        np.testing.assert_array_equal(a, b)
    ref, full = ic.reference('capacity'), ic.reference('plain')
    assert (ref['alpha'] != full['alpha']).any()


@pytest.mark.parametrize('bg_index', [0, 1, 2])
def test_extreme_samples_take_the_branches_they_must(bg_index):
    """h0 = -30: a rounds to 0 in f32, the pixel takes the no-hit branch (alpha 0, depth 0, the background exactly).  h0 = +12, the largest
    finite sigma (h0 = 88.6875) and the f32 infinity (h0 = +89): alpha = 1 to the last ulps, finite everything.  Colours of 1.5 over white clamp
    to 1, colours of -0.25 over black to 0."""
    bg = ic.BACKGROUNDS[bg_index]
    case, marks = ic.extremes(ic.SEEDS['extremes'], bg)
    ref = ic.reference(f'extremes_bg{bg_index}')
    rgb, alpha, depth = _composite(case)
    assert np.isfinite(rgb).all() and np.isfinite(alpha).all() and np.isfinite(depth).all()
    _, _, pix = ic._geometry(case['width'], case['height'], 0, ic.N_TILES)
    p = pix[marks['no_hit']]
    assert (alpha[p] == 0).all() and (depth[p] == 0).all() and (rgb[p] == np.clip(np.asarray(bg, np.float32), 0, 1)).all()
    for key in ('opaque', 'inf', 'huge'):
        p = pix[marks[key]]
        assert (alpha[p] >= 1 - 2.0 ** -20).all() and (alpha[p] <= 1).all(), key
    if min(bg) == 1:
        assert (rgb[pix[marks['above_one']]] == 1).all()
    if max(bg) == 0:
        assert (rgb[pix[marks['below_zero']]] == 0).all()
    assert (ref['budget']['alpha'] < 2e-5).all()


# ------------------------------------------------------------------------------------------------ b. frames, separated from the networks
def _scene(which):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_garden_parity import garden_camera, garden_model, inside_pose
    from tests.test_gpu_render_parity import make_camera, make_model
    if which == 'one cascade':
        model, cam, pose, exponential = make_model(table_amp=4.0), make_camera(61, 45, bg=(1.0, 0.5, 0.25)), scenes.orbit_pose(0.7, 0.4, scenes.LEGO_RADIUS), False
    else:
        model = garden_model(table_amp=40.0 if which == 'garden, saturating' else 2.0)
        cam, pose, exponential = garden_camera(88, 64), inside_pose(0.9, 0.25), True
    return model, cam, pose, exponential, lambda: InstantNGPRenderer(model, EXPONENTIAL_STEPS=exponential)


@pytest.mark.parametrize('which', ['one cascade', 'garden', 'garden, saturating'])
def test_frames_match_the_reference_compositing_of_their_own_network_outputs(which):
    model, cam, pose, exponential, make = _scene(which)
    rows_r = make()
    rows_r.ARENA_IN_PLACE = False      # compact rows: query -> packed, then nrc_ngp_composite_image; the workspace keeps the frame's arrays
    own = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in rows_r.render_image_fused(cam, pose, return_stats=True, early_termination=False).items()}
    ws = next(iter(rows_r._fused_ws.values()))
    rows, nt = own['n_rows'], rows_r.n_image_tiles(cam)
    tile_off = ws['tile_off'].cpu().numpy()
    assert int(tile_off[nt]) == rows > 0
    case = dict(packed=ws['packed'][:rows * 64].cpu().numpy(), ts=ws['ts'][:rows * 64].cpu().numpy(), ray_cnt=ws['ray_cnt'].cpu().numpy(), tile_off=tile_off,
                width=cam.width, height=cam.height, tile_begin=0, n_tiles=nt, cascades=model.cascades, esf=1 / 256 if exponential else 0.0,
                grid_size=model.RESOLUTION, max_samples=rows_r.MAX_SAMPLES, T_threshold=1e-4, bg3=cam.background_color.tolist(), row_capacity=0, arena_rows=0)
    assert case['packed'].dtype == np.float16
    ref = ic.composite_image_f64(*ic.args_of(case), with_budget=True)
    assert len(ref['pix']) == cam.width * cam.height and own['n_samples'] == int(ref['n'].sum())
    has = ref['n'] > 0
    share = float(ref['threshold'][has].mean())
    stopped = float((ref['stop'][has] < ref['n'][has] - 1).mean())
    bud = {k: float(np.median(v)) for k, v in ref['budget'].items()}
    print(f'\n{which}: {int(has.sum())} rays with samples, longest {int(ref["n"].max())}, threshold rays {share:.5f}, stopped early {stopped:.3f}, '
          f'median budgets {bud}, max alpha budget {float(ref["budget"]["alpha"].max()):.3e}')
    assert share <= ic.THRESHOLD_RAY_CAP
    assert has.mean() > 0.2 and (which == 'garden, saturating' or ref['alpha'].std() > 0.02)       # (the saturating picture is opaque nearly everywhere)
    if which == 'garden':
        assert ref['regimes'][1] > 0.1 * ref['regimes'].sum()       # dt = t / 256 between the clamps is exercised
    if which == 'garden, saturating':
        assert stopped > 0.05       # (the share of opaque pixels tests/test_gpu_garden_parity.py asserts for this model)
    default = make().render_image_fused(cam, pose, early_termination=False)       # nrc_ngp_render_frame: composited inside the MLP kernel
    pictures = {'compact rows': own, 'single pass': {k: v.clone() for k, v in default.items()}}
    pictures['slab order'] = make().render_image_fused(cam, pose, early_termination=True)
    for label, pic in pictures.items():
        _judge(tuple(pic[k].cpu().numpy() for k in ('rgb', 'alpha', 'depth')), ref, f'{which}, {label}')
