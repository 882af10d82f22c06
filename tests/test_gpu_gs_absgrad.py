"""GPU: the absolute screen-space gradients of the 3DGS rasterizer (absgrad=True; k_render_bw<., true>, C ABI nrc_gs_backward_absgrad_band).

Every element of means2D.absgrad[:, :2] is judged against its own float64 budget (tests/gs_absgrad_ref.py: the reference, and why the budget of the signed
mean2D sums bounds the new sums term by term; held against an independent autograd statement and five planted errors in tests/test_gs_absgrad_ref_cpu.py).
As in tests/test_gpu_gs_grad_budget.py, whose helpers run the calls here, the kernel's saved state is asserted equal to the f32 oracle's, the reference is
built from the kernel's floats, the ambiguous pixels (at most 0.5 %) are masked, and in the same backward every ordinary gradient is judged as well.

  1. budget: thirteen cases, each with its own pixel gradients and with a +-1 checkerboard on every channel (where the signed sum cancels to ~0.3 % of the
     abs sum: a kernel that took |.| after any sum is hundreds of budgets off);
  2. nothing else moves: with and without the flag every ordinary gradient element differs by at most the sum of the two budgets; no .absgrad without the flag;
  3. records: abs, plain, abs, plain at another P, abs -- every backward within budget, the kept record buffer all zeros at the end;
  4. bands: three one-row bands on one leaf accumulate to the frame's absgrad; a Gaussian outside a band gets exact zeros from it;
  5. combinations: camera_grad, the refusals, Gaussians.add_densification_stats(use_absgrad=True), and a checkerboard loss over one wide Gaussian that
     densify_and_prune splits on the abs statistic and leaves alone on the signed one.

Measured on the MI355X: worst err / budget of absgrad over the 26 runs of 1. 0.109 (dense-aux, own gradients), then 0.042 (grad-2^-70) and 0.031 (aux-all, checkerboard), otherwise
0.006 .. 0.019; 0 pixels masked in every case; 2.: the ordinary gradients with and without the flag differ by at most 0.003 of the two budgets (sh); 4.: three bands on one leaf against
the whole frame: 0.003 of a budget; 5.: the wide Gaussian under the checkerboard has |grad| 0.0948 and absgrad 271.2, the threshold between them is 5.07."""
import contextlib
import copy
from unittest import mock

import numpy as np
import pytest
import torch

from tests import gs_absgrad_ref as AR
from tests import gs_grad_cases as C
from tests import gs_grad_ref as R
from tests import scenes
from tests.test_gpu_gs_grad_budget import (DEV, T, _assert_within_budget, _backward, _check_state, _forward, _gradients_of, _kernel_floats, _settings,
                                           _with_device_activations)
from tests.test_gs_absgrad_ref_cpu import checkerboard

pytestmark = pytest.mark.gpu

CASES = ('partial-70x45-deg3', 'partial-9x5', 'full-16x16', 'single-wide', 'dense-aux', 'aux-all', 'grad-tile-exponents', 'grad-2^-70',
         'grad-alternate-tiles-zero', 'grad-one-pixel', 'clamp-alpha-0.999', 'precomp', 'raw-split-sh')
STATE_KEYS = ('radii', 'points_xy', 'conic_opacity', 'rgb', 'clamped', 'cov3D', 'point_list', 'ranges', 'n_contrib', 'depths')


@contextlib.contextmanager
def _flags(**extra):
    """The calls of tests/test_gpu_gs_grad_budget.py's _forward with further keyword arguments for the rasterizer."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    plain = GaussianRasterizer.forward

    def forward(self, *args, **kw):
        return plain(self, *args, **{**extra, **kw})

    with mock.patch.object(GaussianRasterizer, 'forward', forward):
        yield


_STATES = {}


def _entry(c):
    """Per case: the f32 oracle's state and, from the first call on, the kernel's state and the float64 forward decisions built from it (shared, never modified)."""
    if isinstance(c, str):
        if c not in _STATES:
            case = C.get(c)
            _STATES[c] = dict(c=_with_device_activations(case) if case.form == 'raw' else case)
        return _STATES[c]
    return _STATES.setdefault(c.name, dict(c=c))


def _call(case, grads=None, absgrad=True, key=None):
    """Forward (with the flag), the reference for `grads` (default: the case's own), backward.  Returns (c, r, leaves)."""
    e = _entry(case)
    c = e['c']
    with (_flags(absgrad=True) if absgrad else contextlib.nullcontext()):
        out, leaves, state = _forward(c)
    if 'first' not in e:
        e['st'] = C.forward(c)[0]
        _check_state(e['st'], state)
        e['st64'] = R.promote(e['st'], **_kernel_floats(e['st'], state))
        e['blend'] = R.BlendRef(e['st64'], c.bg, aux=bool(c.aux))
        e['first'] = state
    for k in STATE_KEYS:
        np.testing.assert_array_equal(state[k], e['first'][k])
    refs = e.setdefault('refs', {})
    if key is None or key not in refs:
        r = C.reference_for(c, e['st64'], e['blend'], grads)
        r.want_abs = AR.want_abs(r.blend, *((r.g, r.g_d, r.g_a) if c.aux else (r.g,)))
        if key is not None:
            refs[key] = r
    else:
        r = refs[key]
    _backward(c, out, r)
    return c, r, leaves


def _judge_abs(c, r, absgrad, like, label=''):
    assert torch.is_tensor(absgrad) and tuple(absgrad.shape) == (c.n, 3) and absgrad.dtype == torch.float32 and absgrad.device == like.device
    got = absgrad.cpu().numpy()
    assert np.isfinite(got).all() and not got[:, 2].any()
    A, B = AR.magnitude(r.ref), AR.budget(r.B)
    worst, over, nonzero = AR.judge(got, r.want_abs, B, A)
    print(f'{label}{c.name} absgrad: worst err / budget {worst:.3f}, {over} of {int((A > 0).sum())} over budget, {nonzero} of {int((A == 0).sum())} A == 0 elements not zero')
    assert over == 0 and nonzero == 0, (c.name, worst, over, nonzero)
    return got


# ---------------------------------------------------------------------------------------------------- 1. budget
@pytest.mark.parametrize('kind', ['own', 'checkerboard'])
@pytest.mark.parametrize('name', CASES)
def test_1_every_absgrad_element_within_its_budget(name, kind):
    c = _entry(name)['c']
    c, r, leaves = _call(name, None if kind == 'own' else checkerboard(c), key=kind)
    print(f'{name} / {kind}: {r.masked} of {c.w * c.h} pixels masked')
    got = _judge_abs(c, r, leaves['mean2D'].absgrad, leaves['mean2D'], f'{kind}: ')
    live = r.want_abs > 0
    assert live.sum() >= 1
    if kind == 'checkerboard' and name == 'partial-70x45-deg3':     # what the kernel returned is the abs sum, far from the signed one
        S = np.abs(r.ref['S'][:, 4:6])
        assert ((got[:, :2] - S > 100 * AR.budget(r.B)) & live).sum() >= 0.5 * live.sum()
    _assert_within_budget(c, _gradients_of(c, leaves), r, label=f'{kind}: ')


# ---------------------------------------------------------------------------------------------------- 2. nothing else moves
def test_2_the_flag_leaves_every_other_gradient_within_the_two_budgets():
    name = 'partial-70x45-deg3'
    c, r, flagged = _call(name, key='own')
    _, _, plain = _call(name, absgrad=False, key='own')
    assert not hasattr(plain['mean2D'], 'absgrad') and hasattr(flagged['mean2D'], 'absgrad')
    a, b = _gradients_of(c, flagged), _gradients_of(c, plain)
    _assert_within_budget(c, b, r, label='plain: ')
    for leaf in C.leaf_names(c):
        diff = np.abs(np.asarray(a[leaf], np.float64) - np.asarray(b[leaf], np.float64)).reshape(r.leaf.budget[leaf].shape)
        assert (diff <= 2 * r.leaf.budget[leaf]).all(), leaf                          # (A == 0: budget 0, both exactly zero)
        print(f'{leaf}: largest |with - without| / (2 budget) = {np.where(r.leaf.A[leaf] > 0, diff / np.where(r.leaf.A[leaf] > 0, 2 * r.leaf.budget[leaf], 1), 0).max():.3f}')


# ---------------------------------------------------------------------------------------------------- 3. records
def test_3_records_stay_clear_across_abs_and_plain_backward_passes():
    from nerficg_amd import diff_gaussian_rasterization as dgr
    big = _entry('partial-70x45-deg3')['c']
    small = copy.copy(big)
    small.sc = {k: (v[:200].copy() if isinstance(v, np.ndarray) else v) for k, v in big.sc.items()}
    small.n, small.name = 200, 'first 200 Gaussians'
    for step, (case, seed, flag) in enumerate(((big, 1, True), (big, 2, False), (big, 3, True), (small, 4, False), (big, 1, True))):
        c, r, leaves = _call(case.name if case is big else case, C.pixel_gradients(case, seed=seed), absgrad=flag)
        label = f'backward {step + 1} ({"abs" if flag else "plain"}): '
        _assert_within_budget(c, _gradients_of(c, leaves), r, label=label)
        if flag:
            _judge_abs(c, r, leaves['mean2D'].absgrad, leaves['mean2D'], label)
        else:
            assert not hasattr(leaves['mean2D'], 'absgrad')
    kept = [buf for rows, buf in dgr._GRAD_RECORDS.values() if rows == big.n]
    assert kept and all(tuple(buf.shape) == (big.n, 16) and not bool(buf.any()) for buf in kept)      # slots [10], [11] included


# ---------------------------------------------------------------------------------------------------- 4. bands
def _leaves_of(c):
    sc = c.sc
    return dict(means3D=T(sc['means3D']).requires_grad_(True), opacities=T(sc['opacities'])[:, None].requires_grad_(True), shs=T(sc['shs']).requires_grad_(True),
                scales=T(sc['scales']).requires_grad_(True), rotations=T(sc['rotations']).requires_grad_(True))


def test_4_band_shares_accumulate_on_one_leaf_to_the_frame():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer, last_band_mask
    name = 'partial-70x45-deg3'
    c, r, frame = _call(name, key='own')
    whole = _judge_abs(c, r, frame['mean2D'].absgrad, frame['mean2D'], 'frame: ')
    assert (c.h + 15) // 16 == 3
    m2 = torch.zeros(c.n, 3, device=DEV, requires_grad=True)
    alone, masks = [], []
    for row in range(3):
        single = torch.zeros(c.n, 3, device=DEV, requires_grad=True)
        for leaf in (m2, single):
            image, radii = GaussianRasterizer(_settings(c))(means2D=leaf, tile_rows=(row, 1), absgrad=True, **_leaves_of(c))
            mask = last_band_mask()
            image.backward(T(r.g))
        alone.append(single.absgrad.cpu().numpy())
        masks.append(mask.cpu().numpy().astype(bool))
        outside = (radii.cpu().numpy() > 0) & ~masks[-1]
        assert outside.sum() >= 1 and not alone[-1][outside].any() and not alone[-1][radii.cpu().numpy() <= 0].any()      # exact zeros from a band that misses the Gaussian
    got = _judge_abs(c, r, m2.absgrad, m2, 'three bands on one leaf: ')
    assert m2.grad is not None and not got[:, 2].any()
    total = sum(a.astype(np.float64) for a in alone)
    assert (np.abs(total[:, :2] - r.want_abs) <= AR.budget(r.B)).all()
    print(f'largest |bands - frame| / budget = {np.where(r.want_abs > 0, np.abs(got[:, :2] - whole[:, :2]) / np.where(r.want_abs > 0, AR.budget(r.B), 1), 0).max():.3f}')


# ---------------------------------------------------------------------------------------------------- 5. combinations
def test_5_camera_gradients_are_those_of_the_call_without_the_flag():
    import oracle
    from tests.gs_pose_grad_ref import expected_camera_gradients
    from tests.test_gpu_gs_pose_grad import CASES as POSE_CASES, _camera_grads, _check, _oracle, _pixel_gradient, _run, _scene
    key = POSE_CASES['scene A']
    sc, cam = _scene(*key)
    _, _, st, _ = _oracle(key)
    g = _pixel_gradient(cam['height'], cam['width'], 3)
    want = expected_camera_gradients(sc, cam, st, oracle.gs_backward(st, g))
    runs = {}
    for flag in (False, True):
        runs[flag] = _run(sc, cam, absgrad=flag)
        runs[flag]['out'][0].backward(T(g))
        _check(_camera_grads(runs[flag]), want, label=f'absgrad={flag}: ')
    assert torch.equal(runs[True]['out'][0], runs[False]['out'][0])
    absgrad = runs[True]['leaves']['means2D'].absgrad
    signed = runs[True]['leaves']['means2D'].grad
    assert tuple(absgrad.shape) == tuple(signed.shape) and float(absgrad[:, :2].sum()) > float(signed[:, :2].abs().sum()) > 0 and not bool(absgrad[:, 2].any())
    assert not hasattr(runs[False]['leaves']['means2D'], 'absgrad')


def test_5_rest_step_and_features_are_refused():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    from nerficg_amd.gaussian_splatting import render_image_training
    from tests.test_gpu_gs_pose_grad import _gaussians, _perspective
    c = C.get('partial-70x45-deg3')
    t = {k: T(v) for k, v in c.sc.items() if k != 'sh_degree'}

    class Step:
        def take(self):
            raise AssertionError('the step must not be taken')

    common = dict(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None], scales=t['scales'], rotations=t['rotations'])
    with pytest.raises(RuntimeError, match='absgrad together with rest_step'):
        GaussianRasterizer(_settings(c))(shs=t['shs'][:, :1].contiguous(), shs_rest=t['shs'][:, 1:].contiguous(), rest_step=Step(), absgrad=True, **common)
    with pytest.raises(RuntimeError, match='absgrad together with features.*another kernel'):
        GaussianRasterizer(_settings(c))(shs=t['shs'], features=torch.ones(c.n, 4, device=DEV), absgrad=True, **common)
    g = _gaussians(c.sc)
    g.training_setup(training_cameras_extent=3.0)
    cam, c2w = _perspective(c.w, c.h), scenes.orbit_pose(*C.POSE)
    with pytest.raises(RuntimeError, match='absgrad'):
        render_image_training(g, cam, c2w, fuse_rest_step=True, absgrad=True)
    g.fuse_rest_step = True                                       # the model's own default: resolves to "not fused" with the flag
    out = render_image_training(g, cam, c2w, absgrad=True)
    out['rgb'].sum().backward()
    assert tuple(out['viewspace_points'].absgrad.shape) == (c.n, 3) and g._features_rest.grad is not None


def test_5_densification_statistics_from_absgrad():
    from nerficg_amd.gaussian_splatting import render_image_training
    from tests.test_gpu_gs_pose_grad import _gaussians, _perspective
    c = C.get('partial-70x45-deg3')
    g = _gaussians(c.sc)
    g.training_setup(training_cameras_extent=3.0)
    out = render_image_training(g, _perspective(c.w, c.h), scenes.orbit_pose(*C.POSE), absgrad=True)
    plain = render_image_training(g, _perspective(c.w, c.h), scenes.orbit_pose(*C.POSE))
    with pytest.raises(RuntimeError, match='absgrad'):
        g.add_densification_stats(plain['viewspace_points'], plain['radii'], use_absgrad=True)      # no backward, no flag: nothing to read
    (out['rgb'] * T(checkerboard(c)[0])).sum().backward()
    vsp, radii = out['viewspace_points'], out['radii']
    before, n_before = g.densification_gradient_accum.cpu().numpy().copy(), g.n_observations.cpu().numpy().copy()
    g.add_densification_stats(vsp, radii, use_absgrad=True)
    a = vsp.absgrad.cpu().numpy()
    vis = radii.cpu().numpy() > 0
    assert vis.sum() > 100 and (a[vis, :2] > 0).any()
    norms = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(np.float32))
    want = before[:, 0] + np.where(vis, norms, np.float32(0))
    np.testing.assert_allclose(g.densification_gradient_accum.cpu().numpy()[:, 0], want, rtol=1e-6, atol=0)
    np.testing.assert_array_equal(g.n_observations.cpu().numpy()[:, 0], n_before[:, 0] + vis)


def test_5_a_checkerboard_over_one_wide_gaussian_splits_on_the_abs_statistic_only():
    """One splat of sigma ~ 3 pixels under a +-1 checkerboard loss: the per-pixel terms of dL/dmean2D alternate in sign and cancel in .grad, not in .absgrad.  The
    threshold is the geometric mean of the two measured statistics."""
    from nerficg_amd.gaussian_splatting import render_image_training
    from tests.test_gpu_gs_pose_grad import _gaussians, _perspective, _single
    sc, cam = _single('wide')
    c = C.get('single-wide')
    info, stat = {}, {}
    for use_abs in (False, True):
        g = _gaussians(sc)
        g.training_setup(training_cameras_extent=3.0)
        out = render_image_training(g, _perspective(32, 32), scenes.orbit_pose(*C.POSE), absgrad=True)
        (out['rgb'] * T(checkerboard(c)[0])).sum().backward()
        vsp = out['viewspace_points']
        assert int(out['radii'][0]) > 0
        signed, absolute = float(vsp.grad[0, :2].norm()), float(vsp.absgrad[0, :2].norm())
        assert absolute > 10 * signed > 0, (signed, absolute)
        threshold = float(np.sqrt(signed * absolute))
        g.add_densification_stats(vsp, out['radii'], use_absgrad=use_abs)
        stat[use_abs] = float(g.densification_gradient_accum[0, 0])
        info[use_abs] = g.densify_and_prune(grad_threshold=threshold, min_opacity=0.005, prune_large_gaussians=False)
        print(f'use_absgrad={use_abs}: statistic {stat[use_abs]:.4e} (signed {signed:.4e}, abs {absolute:.4e}), threshold {threshold:.4e}, {info[use_abs]}')
    assert info[False]['n_split'] == 0 and info[False]['n_cloned'] == 0 and info[False]['n_out'] == 1
    assert info[True]['n_split'] == 1 and info[True]['n_out'] == 2
