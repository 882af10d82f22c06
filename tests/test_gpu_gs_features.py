"""GPU: N-channel per-Gaussian features blended by the 3DGS rasterizer (GaussianRasterizer(..., features=); C ABI nrc_gs_render_features_band /
nrc_gs_backward_features_band; kernels k_render_features / k_render_features_bw in nerficg_amd/csrc/gs_features.hip).

Reference and budgets: tests/gs_features_ref.py (derivation in its docstring; held against the float64 oracle, a central difference and the float32 oracle in
tests/test_gs_features_ref_cpu.py), built on the kernel's own saved state as tests/test_gpu_gs_grad_budget.py does.  Every element of the map, of
features.grad and of every leaf gradient is judged against its own budget where its magnitude A is positive and must be exactly zero where A is zero; the
budget tests print the worst error / budget per tensor.

The backward cases run at C = 17 (two chunks, the second a single channel, rows that are not 16-byte aligned) -- the 2000-Gaussian case at C = 5, to keep its
float64 reference to two runs -- and the base case also at C = 1, 5 and 16 (one chunk; 16 takes the 16-byte loads); the pixel-gradient kinds run at C = 5."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import gs_features_ref as F
from tests import gs_grad_cases as GC
from tests import gs_grad_ref as R
from tests import scenes
from tests import test_gpu_gs_grad_budget as BT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = BT.T
BASE = 'partial-70x45-deg3'
MAP_CASES = (BASE, 'partial-9x5', 'full-16x16', 'dense-plain', 'clamp-alpha-0.999', 'single-wide')
BW_CASES = MAP_CASES + ('partial-113x71-2000-deg2', 'raw-split-sh', 'precomp', 'scale-modifier-0.7')


def _case(name):
    c = GC.get(name)
    return BT._with_device_activations(c) if c.form == 'raw' else c


def _forward(c, feats, feat_grad=True, **kw):
    """BT._forward with `features`.  Returns (outputs, leaves, state, the features leaf)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    sc = c.sc
    leaf = lambda a: T(a).requires_grad_(True)
    m3, m2 = leaf(sc['means3D']), torch.zeros(c.n, 3, device=DEV, requires_grad=True)
    if c.form == 'raw':
        raw = sc['raw']
        op, dc, rest, ls, qt = (leaf(raw[k]) for k in ('logit', 'dc', 'rest', 'log_scale', 'quat'))
        leaves = dict(mean3D=m3, mean2D=m2, opacity=op, scale=ls, rot=qt, sh=(dc, rest))
        args = dict(opacities=op, shs=dc, shs_rest=rest, scales=ls, rotations=qt, raw_parameters=True)
    elif c.form == 'precomp':
        op, col, cov = leaf(sc['opacities']), leaf(sc['colors_precomp']), leaf(sc['cov3D_precomp'])
        leaves = dict(mean3D=m3, mean2D=m2, opacity=op, color=col, cov3D=cov)
        args = dict(opacities=op[:, None], colors_precomp=col, cov3D_precomp=cov)
    else:
        op, sh, s, q = leaf(sc['opacities']), leaf(sc['shs']), leaf(sc['scales']), leaf(sc['rotations'])
        leaves = dict(mean3D=m3, mean2D=m2, opacity=op, scale=s, rot=q, sh=sh)
        args = dict(opacities=op[:, None], shs=sh, scales=s, rotations=q)
    ft = None if feats is None else T(feats).requires_grad_(feat_grad)
    if ft is not None:
        kw['features'] = ft
    out = GaussianRasterizer(kw.pop('settings', None) or BT._settings(c))(means3D=m3, means2D=m2, **args, **kw)
    fn = out[0].grad_fn
    state = None                                           # (under no_grad there is no node to read the saved state from)
    if fn is not None:
        state = {k: v.detach().cpu().numpy() for k, v in zip(BT.SAVED, fn.saved_tensors)}
        state['depths'] = fn.debug_state['depths'].detach().cpu().numpy()
        state['num_rendered'] = int(fn.num_rendered)
    return out, leaves, state, ft


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, f32 oracle state, promoted kernel state, BlendRef with bg = 0): once per case, from the kernel's own saved state, never modified."""
    c = _case(name)
    st, _ = GC.forward(c)
    out, leaves, state, _ = _forward(c, None)
    BT._check_state(st, state)
    st64 = R.promote(st, **BT._kernel_floats(st, state))
    blend = R.BlendRef(st64, np.zeros(3))
    masked = int(blend.ambiguous.sum())
    assert masked <= 0.005 * c.w * c.h, f'{masked} of {c.w * c.h} pixels are ambiguous'
    return c, st, st64, blend


@functools.lru_cache(maxsize=None)
def _feature_ref(name, C, kind='normal'):
    """(FeatureRef, features, masked map gradients, sums, B, BF) of a case: computed once, shared, never modified."""
    c, st, st64, blend = _built(name)
    feats = F.random_features(c.n, C, seed=C)
    fr = F.FeatureRef(blend, feats)
    g = fr.mask_ambiguous(F.random_map_gradients(c, C, kind=kind, seed=C))
    ref = fr.sums(g)
    B, BF = F.budget(ref)
    return fr, feats, g, ref, B, BF


@functools.lru_cache(maxsize=None)
def _colour_ref(name):
    c, st, st64, blend = _built(name)
    blend_c = copy.copy(blend)
    blend_c.bg = np.asarray(c.bg, np.float64).reshape(3)
    return GC.reference_for(c, st64, blend_c)


def _judge(label, got, want, budget, A):
    worst, over, nonzero = R.judge(got, want, budget, A)
    print(f'{label}: worst err / budget {worst:.3f}, {over} of {int((A > 0).sum())} over budget, {nonzero} of {int((A == 0).sum())} A == 0 elements not zero')
    assert over == 0 and nonzero == 0, (label, worst, over, nonzero)


# ------------------------------------------------------------------------------------------------------------------------ 1. the colour's own weights
def _plain_scene(n, w, h, seed):
    import math
    if n == 'dense':
        from tests.test_gpu_gs_depth_alpha import _dense_scene
        return _dense_scene()
    sc = scenes.gs_random_scene(n, seed=seed, extent=1.2, log_scale_mean=math.log(0.03), sh_degree=0)
    return sc, scenes.gs_camera(w, h, scenes.orbit_pose(0.9 + seed, 0.35, 3.2))


def _channels_from(col, C):
    """(features (P, C), the image plane each channel must equal)."""
    if C == 3:
        planes = [0, 1, 2]
    elif C == 6:
        planes = [0, 1, 2, 2, 1, 0]
    elif C == 17:
        planes = [k % 3 for k in range(16)] + [0]
    else:
        planes = [k % 3 for k in range(C)]
    return np.ascontiguousarray(col[:, planes]), planes


@pytest.mark.parametrize('C', [3, 6, 17, 40])
@pytest.mark.parametrize('n,w,h,seed', [(1, 32, 32, 0), (500, 100, 70, 1), (3000, 64, 48, 3), ('dense', 40, 40, 4)])
def test_feature_planes_are_the_image_planes_bit_for_bit(n, w, h, seed, C):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sc, cam = _plain_scene(n, w, h, seed)
    P = sc['means3D'].shape[0]
    col = np.random.default_rng(50 + seed).random((P, 3)).astype(np.float32)
    feats, planes = _channels_from(col, C)
    rs = GaussianRasterizationSettings(image_height=cam['height'], image_width=cam['width'], tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=torch.zeros(3, device=DEV),
                                       scale_modifier=1.0, viewmatrix=T(cam['viewmatrix']), projmatrix=T(cam['projmatrix']), sh_degree=0, campos=T(cam['campos']),
                                       prefiltered=False, debug=False)
    args = dict(means3D=T(sc['means3D']).requires_grad_(True), means2D=torch.zeros(P, 3, device=DEV), opacities=T(sc['opacities'])[:, None], colors_precomp=T(col),
                scales=T(sc['scales']), rotations=T(sc['rotations']))
    plain = GaussianRasterizer(rs)(**args)
    out = GaussianRasterizer(rs)(**args, features=T(feats))
    assert len(plain) == 2 and len(out) == 3 and out[2].shape == (C, cam['height'], cam['width']) and out[2].dtype == torch.float32
    assert int((out[1] > 0).sum()) >= 1 and bool(out[0].any())
    for k, p in enumerate(planes):
        assert torch.equal(out[2][k], out[0][p]), f'feature plane {k} differs from image plane {p}'
    a, b = plain[0].grad_fn.debug_state, out[0].grad_fn.debug_state
    assert torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])
    assert torch.equal(a['n_contrib'], b['n_contrib']) and torch.equal(a['final_T'], b['final_T'])
    if n == 'dense':
        assert int(b['n_contrib'].max()) > 256                                             # some pixel walks past the first batch


# ------------------------------------------------------------------------------------------------------------------------ 2. the map
@pytest.mark.parametrize('C', [1, 5, 16, 17])
@pytest.mark.parametrize('name', MAP_CASES)
def test_every_map_element_within_its_budget(name, C):
    c, st, st64, blend = _built(name)
    feats = F.random_features(c.n, C, seed=C)
    want, bud, mag = F.FeatureRef(blend, feats).feature_map()
    with torch.no_grad():
        out = _forward(c, feats)[0]
    got = out[-1].cpu().numpy()
    assert np.isfinite(got).all() and (mag > 0).any()
    _judge(f'{name} C={C} map', got, want, bud, mag)


# ------------------------------------------------------------------------------------------------------------------------ 3. the backward
def _run_backward(c, feats, g_map, g_colour=None):
    out, leaves, state, ft = _forward(c, feats)
    if g_colour is None:
        g_colour = np.zeros((3, c.h, c.w), np.float32)
    torch.autograd.backward([out[0], out[-1]], [T(g_colour), T(g_map)])
    return BT._gradients_of(c, leaves), ft.grad.cpu().numpy()


def _assert_backward(name, C, kind='normal'):
    c, st, st64, blend = _built(name)
    fr, feats, g, ref, B, BF = _feature_ref(name, C, kind)
    # the new kernel alone: a zero colour gradient (k_render_bw returns early on every tile)
    got, dfeat = _run_backward(c, feats, g)
    assert (ref['AF'] > 0).any() and (ref['A'][:, 3:] > 0).any()
    _judge(f'{name} C={C} {kind} features.grad', dfeat, ref['SF'], BF, ref['AF'])
    leaf = F.leaves(c, st64, ref, B)
    for k, (worst, over, nonzero) in GC.judge_all(c, got, leaf, label=f'C={C} {kind} features only: ').items():
        assert over == 0 and nonzero == 0, (name, k, worst, over, nonzero)
    # colour and features together, against the budget of the sum
    r = _colour_ref(name)
    got, dfeat = _run_backward(c, feats, g, r.g)
    _judge(f'{name} C={C} {kind} features.grad beside the colour', dfeat, ref['SF'], BF, ref['AF'])
    ref_sum, B_sum = F.combined(ref, B, r.ref, r.B)
    leaf = F.leaves(c, st64, ref_sum, B_sum)
    for k, (worst, over, nonzero) in GC.judge_all(c, got, leaf, label=f'C={C} {kind} colour + features: ').items():
        assert over == 0 and nonzero == 0, (name, k, worst, over, nonzero)


@pytest.mark.parametrize('name', BW_CASES)
def test_every_gradient_element_within_its_budget(name):
    _assert_backward(name, 5 if name == 'partial-113x71-2000-deg2' else 17)


@pytest.mark.parametrize('C', [1, 5, 16])
def test_every_gradient_element_within_its_budget_one_chunk(C):
    _assert_backward(BASE, C)


@pytest.mark.parametrize('kind', ['normal', 'one_pixel', 'tile_exponents', 'hot_pixel', 'tiny', 'alternate_tiles'])
def test_pixel_gradient_kinds(kind):
    _assert_backward(BASE, 5, kind)


# ------------------------------------------------------------------------------------------------------------------------ 4. no feature gradient
def _records_are_clear(n):
    from nerficg_amd import diff_gaussian_rasterization as dgr
    kept = [buf for rows, buf in dgr._GRAD_RECORDS.values() if rows == n]
    assert kept, 'no kept gradient-record buffer of this size'
    assert all(not bool(buf.any()) for buf in kept), 'the kept gradient records are not all zero'


def test_a_missing_or_zero_feature_gradient_changes_nothing():
    """On a frame of ONE tile (full-16x16), where the blend backward's records are reproducible: with several tiles the colour's tile sums reach a record as f32
    atomics in arrival order, and two calls WITHOUT features already differ in their last bits (tests/test_gpu_gs_pose_grad.py states and handles this the
    same way).  The record checks at the end run on the 70 x 45 frame as well."""
    c, st, st64, blend = _built('full-16x16')
    feats = F.random_features(c.n, 17, seed=1)
    g = GC.pixel_gradients(c)[0]
    out, leaves, _, _ = _forward(c, None)
    out[0].backward(T(g))
    plain = BT._gradients_of(c, leaves)
    _records_are_clear(c.n)
    for zero in (False, True):
        out, leaves, _, ft = _forward(c, feats)
        if zero:          # the launch runs and finds no gradient on any tile
            torch.autograd.backward([out[0], out[2]], [T(g), torch.zeros_like(out[2])])
        else:             # the launch is skipped
            out[0].backward(T(g))
        got = BT._gradients_of(c, leaves)
        for k in plain:
            assert np.array_equal(got[k], plain[k]), (k, 'zero' if zero else 'missing')
        assert ft.grad is not None and ft.grad.shape == (c.n, 17) and not bool(ft.grad.any())
        _records_are_clear(c.n)
    # and after a backward that did carry a feature gradient, on one tile and on many
    for name in ('full-16x16', BASE):
        c = _built(name)[0]
        fr, feats, gm, ref, B, BF = _feature_ref(name, 17)
        _run_backward(c, feats, gm, GC.pixel_gradients(c)[0])
        _records_are_clear(c.n)
        _run_backward(c, feats, gm)
        _records_are_clear(c.n)


# ------------------------------------------------------------------------------------------------------------------------ 5. bands
def test_two_bands_compose_the_map_and_share_the_gradient():
    c, st, st64, blend = _built(BASE)                     # 70 x 45: three tile rows, the last 13 pixel rows high
    C = 17
    fr, feats, g, ref, B, BF = _feature_ref(BASE, C)
    with torch.no_grad():
        whole = _forward(c, feats)[0][2]
    total, total_f, summed = None, None, torch.zeros_like(whole)
    want = dict(S=0, A=0)
    Bsum, SF, AF, BFsum = 0, 0, 0, 0
    for band in ((0, 2), (2, 1)):
        y0, y1 = min(c.h, 16 * band[0]), min(c.h, 16 * (band[0] + band[1]))
        out, leaves, _, ft = _forward(c, feats, tile_rows=band)
        part = out[2].detach()
        assert torch.equal(part[:, y0:y1], whole[:, y0:y1]) and not part[:, :y0].any() and not part[:, y1:].any(), band
        summed += part
        gb = np.zeros_like(g)
        gb[:, y0:y1] = g[:, y0:y1]
        torch.autograd.backward([out[2]], [T(g)])                                           # the whole gradient: the band reads its own rows only
        got = BT._gradients_of(c, leaves)
        total = got if total is None else {k: total[k] + got[k] for k in got}
        total_f = ft.grad.cpu().numpy() if total_f is None else total_f + ft.grad.cpu().numpy()
        rb = fr.sums(gb)
        Bb, BFb = F.budget(rb)
        want = dict(S=want['S'] + rb['S'], A=want['A'] + rb['A'])
        Bsum, SF, AF, BFsum = Bsum + Bb, SF + rb['SF'], AF + rb['AF'], BFsum + BFb
    assert torch.equal(summed, whole)
    np.testing.assert_allclose(want['S'], ref['S'], rtol=1e-9, atol=1e-12 * np.abs(ref['S']).max())     # the bands' float64 sums are the frame's
    _judge('bands features.grad', total_f, SF, BFsum, AF)
    leaf = F.leaves(c, st64, want, Bsum)
    for k, (worst, over, nonzero) in GC.judge_all(c, total, leaf, label='two bands: ').items():
        assert over == 0 and nonzero == 0, (k, worst, over, nonzero)


# ------------------------------------------------------------------------------------------------------------------------ 6. composition
def test_output_order_with_depth_and_alpha_and_inside_fixed_capacity():
    from nerficg_amd.diff_gaussian_rasterization import fixed_capacity
    c, st, st64, blend = _built(BASE)
    feats = F.random_features(c.n, 5, seed=5)
    with torch.no_grad():
        plain = _forward(c, feats)[0]
        both = _forward(c, feats, return_depth_alpha=True)[0]
        aux = _forward(c, None, return_depth_alpha=True)[0]
        with fixed_capacity(st.num_rendered + 1024, 0):
            capped = _forward(c, feats)[0]
    assert len(plain) == 3 and len(both) == 5 and len(aux) == 4
    assert both[2].shape == both[3].shape == (c.h, c.w) and both[4].shape == (5, c.h, c.w)
    assert torch.equal(both[4], plain[2]) and torch.equal(both[2], aux[2]) and torch.equal(both[3], aux[3]) and torch.equal(both[0], plain[0])
    assert torch.equal(capped[2], plain[2])
    # gradients through all three kinds of output at once: finite, and the features' part is there
    out, leaves, _, ft = _forward(c, feats, return_depth_alpha=True)
    (out[0].sum() + out[2].sum() + out[3].sum() + (out[4] * out[4]).sum()).backward()
    assert bool(torch.isfinite(ft.grad).all()) and bool(ft.grad.any())
    with fixed_capacity(st.num_rendered + 1024, 0):
        out, leaves, _, ft = _forward(c, feats)
        out[2].backward(T(F.random_map_gradients(c, 5, seed=5)))
    fr, feats5, g, ref, B, BF = _feature_ref(BASE, 5)
    assert np.array_equal(feats5, feats)
    out, leaves, _, ft2 = _forward(c, feats)
    out[2].backward(T(F.random_map_gradients(c, 5, seed=5)))
    np.testing.assert_allclose(ft.grad.cpu().numpy(), ft2.grad.cpu().numpy(), rtol=0, atol=2 * float(np.abs(BF).max()))


def test_camera_gradient_of_a_features_only_loss():
    """The pose reference of tests/gs_pose_grad_ref.py fed with the total per-Gaussian sums of the feature reference, judged as test_gpu_gs_pose_grad.py judges."""
    from tests import test_gpu_gs_pose_grad as PG
    from tests.gs_pose_grad_ref import expected_camera_gradients
    c, st, st64, blend = _built(BASE)
    fr, feats, g, ref, B, BF = _feature_ref(BASE, 17)
    leaf = F.leaves(c, st64, ref, B)
    rs = PG._settings(c.cam, c.sc['sh_degree'], bg=c.bg)
    out, leaves, _, ft = _forward(c, feats, settings=rs, camera_grad=True)
    out[2].backward(T(g))
    grads = dict(mean2D=leaf.want['mean2D'], conic=leaf.want['conic'], mean3D=leaf.want['mean3D'], color=np.zeros((c.n, 3)))
    want = expected_camera_gradients(c.sc, c.cam, st, grads)
    PG._check({k: getattr(rs, k).grad for k in PG.CAMERA}, want, label='features only: ')
    assert np.abs(want['view'][0]).max() > 0 and np.abs(want['proj'][0]).max() > 0 and not np.abs(want['campos'][0]).any()


def test_rest_step_and_malformed_features_raise():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    c = _case(BASE)
    sc = c.sc
    t = {k: T(v) for k, v in sc.items() if isinstance(v, np.ndarray)}
    rast = GaussianRasterizer(BT._settings(c))
    base = dict(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None], scales=t['scales'], rotations=t['rotations'])
    ok = T(F.random_features(c.n, 4))

    class Step:
        def take(self):
            raise AssertionError('the step must not be taken')

    with pytest.raises(RuntimeError, match='features.*rest_step'):
        rast(**base, shs=t['shs'][:, :1].contiguous(), shs_rest=t['shs'][:, 1:].contiguous(), rest_step=Step(), features=ok)
    for bad, err in ((ok[:-1], ValueError), (ok[:, 0], ValueError), (ok.double(), ValueError), (ok.cpu(), RuntimeError), (ok[:, :0], ValueError),
                     (torch.zeros(c.n, 257, device=DEV), ValueError), (ok.cpu().numpy(), ValueError)):
        with pytest.raises(err, match='features'):
            rast(**base, shs=t['shs'], features=bad)
    out = rast(**base, shs=t['shs'], features=ok.t().contiguous().t())                      # a non-contiguous view is accepted (copied)
    assert torch.equal(out[2], rast(**base, shs=t['shs'], features=ok)[2])


# ------------------------------------------------------------------------------------------------------------------------ 7. the renderer mirrors
def test_renderer_mirrors_return_the_map_and_fit_a_target():
    from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera, render_image_inference, render_image_training
    W, H, C = 64, 48, 8
    cam = PerspectiveCamera(W, H, 1.2 * W, 1.2 * W, background_color=torch.tensor([0.1, 0.2, 0.3], device=DEV))
    pose = scenes.orbit_pose(0.4, 0.3, 3.0)
    sc = scenes.gs_random_scene(2000, seed=1, extent=1.0, log_scale_mean=np.log(0.05))
    t = {k: T(v) for k, v in sc.items() if k != 'sh_degree'}
    g = Gaussians(t['means3D'], torch.log(t['scales']), t['rotations'], torch.logit(t['opacities'].clamp(1e-4, 1 - 1e-4))[:, None],
                  t['shs'][:, :1].contiguous(), t['shs'][:, 1:].contiguous())
    g.training_setup(training_cameras_extent=3.0)
    feats = T(F.random_features(2000, C, seed=2)).requires_grad_(True)
    assert 'features' not in render_image_training(g, cam, pose)
    with torch.no_grad():
        target = render_image_training(g, cam, pose, features=T(F.random_features(2000, C, seed=3)))['features'].clone()
        trained = render_image_training(g, cam, pose, features=feats)['features']
    assert target.shape == (C, H, W)
    hwc = render_image_inference(g, cam, pose, features=feats)
    chw = render_image_inference(g, cam, pose, features=feats, to_chw=True)
    assert hwc['features'].shape == (H, W, C) and chw['features'].shape == (C, H, W)
    # The training render hands the kernels raw parameters (exp, sigmoid and the normalisation run inside k_preprocess), the inference render torch's
    # activations: the two geometries differ in the last bits, so the maps are held to the forward parity gate of the project (2e-5 for a channel of order 1,
    # tests/test_gpu_gs_parity.py) times the largest |feature|; the two layouts of the inference render are the same numbers exactly.
    assert torch.equal(hwc['features'], chw['features'].permute(1, 2, 0))
    diff, fmax = float((chw['features'] - trained).abs().max()), float(feats.detach().abs().max())
    print('inference against training render: largest difference', diff, 'bound', 2e-5 * fmax)
    assert diff <= 2e-5 * fmax
    assert torch.equal(chw['rgb'], render_image_inference(g, cam, pose, to_chw=True)['rgb'])
    opt = torch.optim.Adam([feats, g._opacities], lr=0.05)
    losses = []
    for _ in range(12):
        opt.zero_grad(set_to_none=True)
        out = render_image_training(g, cam, pose, features=feats)
        loss = ((out['features'] - target) ** 2).mean()
        loss.backward()
        assert feats.grad is not None and g._opacities.grad is not None and bool(g._opacities.grad.any())
        opt.step()
        losses.append(float(loss))
    print('feature fit: loss', losses[0], '->', losses[-1])
    assert losses[-1] < losses[0]
    with pytest.raises(RuntimeError, match='features'):
        render_image_training(g, cam, pose, fuse_rest_step=True, features=feats)
