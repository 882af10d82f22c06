"""GPU: every element of every gradient of the 3DGS rasterizer backward (k_render_bw, k_preprocess_bw) against its own float64 budget.

Each case (tests/gs_grad_cases.py) runs the drop-in GaussianRasterizer, reads the kernel's saved state from grad_fn, asserts radii, ranges, point_list,
n_contrib and the clamp flags equal to the f32 oracle's, builds the float64 reference and the budgets from THAT state (tests/gs_grad_ref.py: derivation
in its docstring; held against the double oracle, the f32 oracle and eight planted errors in tests/test_gs_grad_ref_cpu.py), zeroes the pixel gradients
of the ambiguous pixels (at most 0.5 %), calls backward and judges every element of every leaf: within its budget where its magnitude A is positive,
exactly zero where A is zero (culled Gaussians, Gaussians no pixel blended, clamped SH channels, SH coefficients above the active degree, means2D[:, 2]).

Measured on the MI355X (worst err / budget per leaf over all cases and the four backward passes of the record test, and the case that sets it):
    means3D 0.80 (partial-9x5)    means2D 0.28 (dense-plain)    opacities 0.13 (partial-113x71-2000-deg2)    scales 0.92 (partial-9x5)
    rotations 0.94 (partial-9x5)    shs 0.08 (full-16x16)    colors_precomp 0.04 (precomp)    cov3D_precomp 0.44 (precomp)
At 9 x 5 every Gaussian is large against the image and its conic sums are small: the budget there is almost all `fixed`, the one truncation step per
depositing (tile, block) pair, a hard bound that truncation toward zero uses about half of on average.  At most 1 pixel of a case is masked as ambiguous.

These tests found that `deposit` of k_render_bw lost 8 bits of the low word of every NEGATIVE row sum (its float32 remainder 2^32 + t rounds to a multiple
of 256: up to 128 steps per deposit instead of less than one): the conic sums, whose step is 2^-25 of the tile's largest pixel gradient, carried errors of
2^-18 of it, and scales, rotations, cov3D_precomp and means3D were up to 113 x over budget in 19 of the 21 cases (worst: dense-aux rotations 113,
partial-113x71-2000-deg2 rotations 97, partial-9x5 rotations 95; colours, opacities and means2D, whose steps are 2^-51 .. 2^-39, stayed inside).  Every
per-tensor 2e-3 gate passed throughout.  The conversion now takes the low word from a remainder in [-2^31, 2^31].
"""
import copy

import numpy as np
import pytest
import torch

from tests import gs_grad_cases as C
from tests import gs_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SAVED = ('means3D', 'sh', 'col', 'sc', 'rot', 'cov', 'radii', 'points_xy', 'conic_opacity', 'rgb', 'clamped', 'cov3D', 'point_list', 'ranges', 'n_contrib', 'final_T')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _settings(c):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = c.cam
    return GaussianRasterizationSettings(
        image_height=c.h, image_width=c.w, tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=T(c.bg), scale_modifier=c.scale_modifier,
        viewmatrix=T(cam['viewmatrix']), projmatrix=T(cam['projmatrix']), sh_degree=c.sc['sh_degree'], campos=T(cam['campos']), prefiltered=False, debug=False)


def _with_device_activations(c):
    """The raw case with the activations formed on the device, in the kernel's operation order, so that the oracle sees the geometry the kernel sees."""
    raw = c.sc['raw']
    act, norm = C.activate({k: T(v) for k, v in raw.items()}, xp=torch)
    c = copy.copy(c)
    c.sc = C.with_activations(raw, {k: v.cpu().numpy() for k, v in act.items()}, norm.cpu().numpy())
    return c


def _forward(c):
    """One call on fresh leaves.  Returns (outputs, {oracle name: leaf tensor or tuple of leaf tensors}, the kernel's saved state as float32 / integer numpy arrays)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    sc = c.sc
    leaf = lambda a: T(a).requires_grad_(True)
    m3, m2, kw = leaf(sc['means3D']), torch.zeros(c.n, 3, device=DEV, requires_grad=True), {}
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
    if c.aux:
        kw['return_depth_alpha'] = True
    out = GaussianRasterizer(_settings(c))(means3D=m3, means2D=m2, **args, **kw)
    assert len(out) == (4 if c.aux else 2)
    fn = out[0].grad_fn
    state = {k: v.detach().cpu().numpy() for k, v in zip(SAVED, fn.saved_tensors)}
    state['depths'] = fn.debug_state['depths'].detach().cpu().numpy()
    state['num_rendered'] = int(fn.num_rendered)
    return out, leaves, state


def _check_state(st, state):
    """The decisions of the kernel are the f32 oracle's: the reference may take the lists and n_contrib as given."""
    P, n = st.P, st.num_rendered
    np.testing.assert_array_equal(state['radii'].reshape(-1)[:P], st.radii)
    np.testing.assert_array_equal(state['ranges'].reshape(-1, 2).astype(np.uint32), st.ranges)
    assert state['num_rendered'] == n
    np.testing.assert_array_equal(state['point_list'].reshape(-1)[:n], st.point_list[:n])
    np.testing.assert_array_equal(state['n_contrib'].reshape(-1).astype(np.uint32), st.n_contrib)
    cl = state['clamped'].reshape(-1)[:P]
    np.testing.assert_array_equal(np.stack([(cl >> ch) & 1 for ch in range(3)], -1), st.clamped)


def _kernel_floats(st, state):
    """The float arrays of the kernel's state, cut to the oracle's shapes."""
    return {k: np.ascontiguousarray(state[k].reshape(-1)[:getattr(st, k).size].reshape(getattr(st, k).shape), np.float32)
            for k in ('points_xy', 'conic_opacity', 'rgb', 'cov3D', 'depths')}


def _gradients_of(c, leaves):
    got = {}
    for name, t in leaves.items():
        if isinstance(t, tuple):
            assert all(x.grad is not None for x in t), name
            got[name] = torch.cat([x.grad for x in t], 1).cpu().numpy()
        else:
            assert t.grad is not None, name
            got[name] = t.grad.cpu().numpy()
    return got


def _backward(c, out, r):
    if c.aux:
        torch.autograd.backward([out[0], out[2], out[3]], [T(r.g), T(r.g_d), T(r.g_a)])
    else:
        out[0].backward(T(r.g))


def _assert_within_budget(c, got, r, label=''):
    for leaf, (worst, over, nonzero) in C.judge_all(c, got, r.leaf, label).items():
        assert over == 0 and nonzero == 0, (c.name, leaf, worst, over, nonzero)


@pytest.mark.parametrize('name', list(C.CASES))
def test_every_gradient_element_within_its_budget(name):
    c = C.get(name)
    if c.form == 'raw':
        c = _with_device_activations(c)
    st, st2 = C.forward(c)
    out, leaves, state = _forward(c)
    _check_state(st, state)
    r = C.reference(c, st, kernel_state=_kernel_floats(st, state))
    print(f'{name}: {r.masked} of {c.w * c.h} pixels masked')
    _backward(c, out, r)
    _assert_within_budget(c, _gradients_of(c, leaves), r)


def test_reused_gradient_records_are_clear():
    """The per-Gaussian backward clears the accumulator records it reads, and the next backward of the same size reuses the buffer without a clearing launch
    (_GRAD_RECORDS): two backward passes on one scene with different gradients, one with another P (the buffer is replaced), the first scene again.  A record
    that was not cleared shows up as the sum of two runs."""
    from nerficg_amd import diff_gaussian_rasterization as dgr
    big = C.get('partial-70x45-deg3')
    small = copy.copy(big)
    small.sc = {k: (v[:200].copy() if isinstance(v, np.ndarray) else v) for k, v in big.sc.items()}
    small.n, small.name = 200, 'first 200 Gaussians'
    refs = {}
    for step, (c, seed) in enumerate(((big, 1), (big, 2), (small, 3), (big, 1))):
        out, leaves, state = _forward(c)
        if c.name not in refs:
            st, _ = C.forward(c)
            _check_state(st, state)
            st64 = R.promote(st, **_kernel_floats(st, state))
            refs[c.name] = (st, state, st64, R.BlendRef(st64, c.bg))
        st, first, st64, blend = refs[c.name]
        for k in ('points_xy', 'conic_opacity', 'rgb', 'n_contrib', 'point_list'):
            np.testing.assert_array_equal(state[k], first[k])
        r = C.reference_for(c, st64, blend, grads=C.pixel_gradients(c, seed=seed))
        _backward(c, out, r)
        assert any(rows == c.n for rows, _ in dgr._GRAD_RECORDS.values())                     # the buffer the next backward of this size takes
        _assert_within_budget(c, _gradients_of(c, leaves), r, label=f'backward {step + 1}: ')
