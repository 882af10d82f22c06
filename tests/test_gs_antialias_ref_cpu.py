"""CPU: the float64 references of the anti-aliased splats and of the 3-D filter (tests/gs_antialias_ref.py) against central differences, the clamp branch, the
floor margins of every test scene, and the rules of the filter."""
import numpy as np
import pytest

from tests import gs_antialias_ref as AA
from tests import gs_grad_cases as C
from tests import gs_grad_ref as R

CASES = AA.cases()
f64 = np.float64


def _state(name):
    c = CASES[name]()
    st, _ = C.forward(c)
    return c, st


def _comp_of(c, st, means=None, cov=None):
    return AA.comp64(c.sc['means3D'] if means is None else means, st.cov3D if cov is None else cov, c.cam)


def test_the_constants_are_the_float32_ones():
    assert AA.DILATION == float(np.float32(0.3)) and AA.FLOOR == float(np.float32(0.000025))
    assert AA.SQRT_0_2 == float(np.sqrt(0.2))


@pytest.mark.parametrize('name', list(CASES))
def test_every_scene_classifies_every_gaussian_with_ten_budgets_of_margin(name):
    c, st = _state(name)
    q = _comp_of(c, st)
    floor = AA.classify(q, st.radii > 0)
    print(f'{name}: {int((st.radii > 0).sum())} visible, {int(floor.sum())} at the floor, largest rho budget {q.b_rho[st.radii > 0].max():.3g}')
    if name.startswith('needles'):
        assert floor.sum() >= 8 and (q.rho[floor] < 0.01 * AA.FLOOR).all()       # well below the floor
        assert ((st.radii > 0) & ~floor).sum() >= 8
    else:
        assert not floor.any()
        assert (q.rho[st.radii > 0] > 100 * AA.FLOOR).all()                       # well above it


def test_extra_terms_against_central_differences_of_o_comp():
    c, st = _state('p127-40x24-deg3')
    q = _comp_of(c, st)
    vis = st.radii > 0
    o = np.asarray(c.sc['opacities'], f64)
    da, dc, db = AA.extra_abc(q, np.ones(c.n), o)
    val = lambda a0, b, c0: o * AA.Comp(a0, b, c0).comp
    for got, k in ((da, 0), (db, 1), (dc, 2)):
        base = [q.a0, q.b, q.c0]
        h = 1e-6 * np.maximum(np.abs(base[k]), 1e-3)
        up, dn = list(base), list(base)
        up[k], dn[k] = base[k] + h, base[k] - h
        num = (val(*up) - val(*dn)) / (2 * h)
        np.testing.assert_allclose(got[vis], num[vis], rtol=1e-6, atol=1e-7 * np.abs(got[vis]).max())   # (the difference quotient's own error: a step of 1e-9 where b is tiny)


def test_clamp_branch_has_no_extra_gradient_and_a_constant_comp():
    c, st = _state('needles-129-40x24')
    q = _comp_of(c, st)
    floor = AA.classify(q, st.radii > 0)
    assert floor.any()
    assert (q.comp[floor] == np.sqrt(AA.FLOOR)).all()
    extra = np.stack(AA.extra_abc(q, np.ones(c.n), c.sc['opacities']), 1)
    assert (extra[floor] == 0).all() and (extra[(st.radii > 0) & ~floor] != 0).any()
    g, _ = AA.equivalent_conic(q, extra, (st.radii > 0) & ~floor)
    assert (g[floor] == 0).all()


def test_equivalent_conic_solves_the_three_lines():
    c, st = _state('p127-40x24-deg3')
    q = _comp_of(c, st)
    vis = st.radii > 0
    extra = np.stack(AA.extra_abc(q, np.ones(c.n), c.sc['opacities']), 1)
    g, _ = AA.equivalent_conic(q, extra, vis)
    a, b, cc = q.a, q.b, q.c
    denom = a * cc - b * b
    d = 1.0 / (denom * denom + 0.0000001)
    gx, gy, gz = g.T
    lines = np.stack([d * (-cc * cc * gx + 2 * b * cc * gy + (denom - a * cc) * gz), d * (-a * a * gz + 2 * a * b * gy + (denom - a * cc) * gx),
                      d * 2 * (b * cc * gx - (denom + 2 * b * b) * gy + a * b * gz)], 1)
    np.testing.assert_allclose(lines[vis], extra[vis], rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize('name', ['p127-40x24-deg3', 'p129-16x16-precomp'])
def test_leaves_of_the_transformed_sums_against_central_differences(name):
    """L = sum_i w_i o_i comp_i: the blend sums are S_opacity = w and nothing else, so LeafRef(S') must hold dL/dcov3D, dL/dmean3D and dL/dopacity of L --
    checked against central differences of comp64 in float64 (cov3D as the leaf; means through Mx, My)."""
    c, st = _state(name)
    P = c.n
    vis = st.radii > 0
    q = _comp_of(c, st)
    w = np.random.default_rng(3).normal(size=P)
    o = np.asarray(c.sc['opacities'], f64)
    st64 = R.promote(st)
    NQ = 9
    ref = dict(S=np.zeros((P, NQ)), A=np.zeros((P, NQ)), R=np.zeros((P, NQ)), tiles=np.zeros(P, np.int64))
    ref['S'][:, 3], ref['A'][:, 3] = w * vis, np.abs(w) * vis
    ref2, B2 = AA.aa_sums(q, ref, np.zeros((P, NQ)), o, vis)
    leaf = R.LeafRef(st64, ref2, B2)
    np.testing.assert_allclose(leaf.want['opacity'][vis], (w * q.comp)[vis], rtol=1e-14)
    L = lambda means, cov: (w * o * np.where(vis, _comp_of(c, st, means, cov).comp, 0.0))
    cov, means = np.asarray(st.cov3D, f64), np.asarray(c.sc['means3D'], f64)
    for k in range(6):
        h = 1e-6 * np.maximum(np.abs(cov[:, k]), 1e-5)
        up, dn = cov.copy(), cov.copy()
        up[:, k] += h
        dn[:, k] -= h
        num = (L(means, up) - L(means, dn)) / (2 * h)
        scale = np.abs(leaf.want['cov3D'][vis]).max()
        np.testing.assert_allclose(leaf.want['cov3D'][vis, k], num[vis], rtol=2e-5, atol=1e-7 * scale)
    # (a Gaussian outside the 1.3 tan(fov / 2) clamp of the Jacobian sits on a kink whose z-dependence the backward, like upstream's, does not carry)
    from tests.gs_pose_grad_ref import fov_clamped
    smooth = vis & ~fov_clamped(c.sc, c.cam, st)
    assert smooth.sum() >= 100
    for k in range(3):
        h = 1e-6
        up, dn = means.copy(), means.copy()
        up[:, k] += h
        dn[:, k] -= h
        num = (L(up, cov) - L(dn, cov)) / (2 * h)
        scale = np.abs(leaf.want['mean3D'][vis]).max()
        np.testing.assert_allclose(leaf.want['mean3D'][smooth, k], num[smooth], rtol=2e-5, atol=1e-7 * scale)
    # every magnitude carries its gradient, and what must be zero is marked
    for k in ('cov3D', 'mean3D'):
        assert (leaf.A[k][vis] >= np.abs(leaf.want[k][vis]) * (1 - 1e-12)).all()
        assert (leaf.A[k][~vis] == 0).all() and (leaf.want[k][~vis] == 0).all()


def test_budget_of_comp_holds_for_a_float32_restatement():
    """The kernel's statements from (a0, b, c0) on, in numpy float32 on the float64 values rounded once: far inside budget(comp), which also carries the
    roundings in front of them."""
    c, st = _state('p300-40x24-deg3-aux')
    q = _comp_of(c, st)
    vis = st.radii > 0
    f = np.float32
    a0, b, c0 = f(q.a0), f(q.b), f(q.c0)
    a, cc = a0 + f(0.3), c0 + f(0.3)
    det0, det1 = a0 * c0 - b * b, a * cc - b * b
    comp = np.sqrt(np.maximum(f(0.000025), det0 / det1))
    err = np.abs(comp.astype(f64) - q.comp)
    assert (err[vis] <= q.b_comp[vis]).all()
    print(f'worst err / budget of the f32 restatement: {(err[vis] / q.b_comp[vis]).max():.3f}')


# ------------------------------------------------------------------------------------------------------------------------ the 3-D filter
def _views():
    from tests import scenes
    out = []
    for th, fx in ((0.5, 50.0), (2.1, 80.0), (4.0, 50.0)):
        c2w = scenes.orbit_pose(th, 0.3, 3.0)
        out.append(AA.view_block(np.linalg.inv(c2w), fx, fx, 40, 24))
    return np.stack(out)


def test_filter3d_ref_rules():
    views = _views()
    ident = AA.view_block(np.eye(4), 32.0, 32.0, 64, 48)[None]
    # on the optical axis at z = 2: seen, sqrt(0.2) * 2 / 32
    f, seen = AA.filter3d_ref(np.array([[0, 0, 2.0]], np.float32), ident)
    assert seen.all() and f[0] == AA.SQRT_0_2 * 2.0 / 32.0
    # the 1.15 border in x: x / z fx + W / 2 = 1.15 W  <=>  x / z = 0.65 W / fx = 1.3: x = 2.6 at z = 2 is on it (exact in binary: 2.6f / 2 * 32 + 32 vs 73.6)
    pts = np.array([[0, 0, 2.0], [2.5, 0, 2.0], [2.7, 0, 2.0], [0, 0, 0.19], [0, 0, -1.0], [0, 1.9, 2.0], [0, 2.0, 2.0]], np.float32)
    f, seen = AA.filter3d_ref(pts, ident)
    assert seen.tolist() == [True, True, False, False, False, True, False]      # y border: 0.65 H / fy = 0.975, times z = 1.95
    assert (f[~seen] == float(np.float32(f[seen]).max())).all()                   # seen by no view: the largest filter among the seen ones
    # behind every camera and none seen at all: zeros
    f, seen = AA.filter3d_ref(np.array([[0, 0, -5.0]], np.float32), ident)
    assert not seen.any() and (f == 0).all()
    # several views: the minimum of z / fx over the seeing ones
    p = np.zeros((1, 3), np.float32)
    f, seen = AA.filter3d_ref(p, views)
    assert seen.all() and abs(f[0] - AA.SQRT_0_2 * 3.0 / 80.0) < 1e-6
