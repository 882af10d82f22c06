"""GPU: anti-aliased splats (GaussianRasterizer(..., antialiasing=True); C ABI group 27) and the 3-D smoothing filter (nrc_gs_filter3d).

The flag sits in the two per-Gaussian kernels only, so the merged default path is the yardstick: a call with the flag must equal, bit for bit, the call without
it on the compensated opacities (test 1); the compensated opacity and every leaf gradient are held against float64 (tests/gs_antialias_ref.py: comp64, the
extra gradient as an equivalent conic gradient, LeafRef on the transformed sums) inside budgets derived there (tests 2, 3).

Bit-equality of per-Gaussian sums of the blend backward (means2D.grad, means2D.absgrad, the floor-hitting Gaussians' gradients) is asserted for the Gaussians
that at most two tiles deposit into: the blend backward adds one float atomic per tile to a Gaussian's record, two addends commute exactly, three or more do not,
and the default path itself does not reproduce their last bit from run to run.  The other rows are held to the reordering bound gamma(tiles) A.

Measured on the MI355X (worst err / budget over all cases): see DESIGN 3.3g."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import gs_antialias_ref as AA
from tests import gs_grad_cases as C
from tests import gs_grad_ref as R
from tests.test_gpu_gs_grad_budget import SAVED, T, _check_state, _gradients_of, _kernel_floats, _settings, _with_device_activations

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = AA.cases()
ACTIVATED = [n for n in CASES if 'raw' not in n]
f64 = np.float64


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]()
    return _with_device_activations(c) if c.form == 'raw' else c


def _call(c, antialiasing, opacities=None, settings_flag=False, **kw):
    """One call on fresh leaves (tests/test_gpu_gs_grad_budget.py: _forward, plus the flag, replaced opacities and further keywords).  Returns (outputs, leaves,
    the kernel's saved state as numpy arrays, the rasterizer object)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    sc = c.sc
    leaf = lambda a: T(a).requires_grad_(True)
    m3, m2 = leaf(sc['means3D']), torch.zeros(c.n, 3, device=DEV, requires_grad=True)
    if c.form == 'raw':
        assert opacities is None
        raw = sc['raw']
        op, dc, rest, ls, qt = (leaf(raw[k]) for k in ('logit', 'dc', 'rest', 'log_scale', 'quat'))
        leaves = dict(mean3D=m3, mean2D=m2, opacity=op, scale=ls, rot=qt, sh=(dc, rest))
        args = dict(opacities=op, shs=dc, shs_rest=rest, scales=ls, rotations=qt, raw_parameters=True)
    elif c.form == 'precomp':
        op, col, cov = leaf(sc['opacities'] if opacities is None else opacities), leaf(sc['colors_precomp']), leaf(sc['cov3D_precomp'])
        leaves = dict(mean3D=m3, mean2D=m2, opacity=op, color=col, cov3D=cov)
        args = dict(opacities=op[:, None], colors_precomp=col, cov3D_precomp=cov)
    else:
        op, sh, s, q = leaf(sc['opacities'] if opacities is None else opacities), leaf(sc['shs']), leaf(sc['scales']), leaf(sc['rotations'])
        leaves = dict(mean3D=m3, mean2D=m2, opacity=op, scale=s, rot=q, sh=sh)
        args = dict(opacities=op[:, None], shs=sh, scales=s, rotations=q)
    if c.aux:
        kw['return_depth_alpha'] = True
    rs = _settings(c)
    if settings_flag:
        rs = rs._replace(antialiasing=True)
    rast = GaussianRasterizer(rs)
    out = rast(means3D=m3, means2D=m2, **args, **({'antialiasing': True} if antialiasing else {}), **kw)
    fn = out[0].grad_fn
    state = {k: v.detach().cpu().numpy() for k, v in zip(SAVED, fn.saved_tensors)}
    state['depths'] = fn.debug_state['depths'].detach().cpu().numpy()
    state['num_rendered'] = int(fn.num_rendered)
    return out, leaves, state, rast


def _compensated(state, n):
    return np.ascontiguousarray(state['conic_opacity'].reshape(-1, 4)[:n, 3], np.float32)


def _assert_same_frame(a, b, sa, sb, n_out):
    for k in range(n_out):
        assert torch.equal(a[k], b[k]), f'output {k} differs'
    for k in ('radii', 'n_contrib', 'ranges', 'points_xy', 'conic_opacity', 'rgb', 'final_T'):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert sa['num_rendered'] == sb['num_rendered']
    n = sa['num_rendered']
    np.testing.assert_array_equal(sa['point_list'].reshape(-1)[:n], sb['point_list'].reshape(-1)[:n])


# ------------------------------------------------------------------------------------------------------------------------ 1. forward identity
@pytest.mark.parametrize('name', ACTIVATED)
def test_1_the_flag_equals_the_default_call_on_the_compensated_opacities(name):
    c = _case(name)
    out_a, _, st_a, rast_a = _call(c, True)
    comp_op = _compensated(st_a, c.n)
    out_y, _, st_y, rast_y = _call(c, False, opacities=comp_op)
    _assert_same_frame(out_a, out_y, st_a, st_y, 4 if c.aux else 2)
    vis = st_a['radii'].reshape(-1)[:c.n] > 0
    assert vis.any() and (comp_op[vis] < np.asarray(c.sc['opacities'])[vis]).all()          # the flag did something: comp < 1 for every visible Gaussian
    # contributions(): the three statistics of the two frames
    ca, cy = rast_a.contributions(), rast_y.contributions()
    for k in ('weight_max', 'hits'):
        assert torch.equal(ca[k], cy[k]), k
    # weight_sum is a sum of float atomics whose order is not fixed even inside one tile (contributions(): "two runs agree to rounding"): its addends are
    # non-negative, so two orders of the `hits` addends differ by at most 2 gamma(hits) of the sum
    wa, wy, hits = ca['weight_sum'].cpu().numpy().astype(f64), cy['weight_sum'].cpu().numpy().astype(f64), ca['hits'].cpu().numpy()
    assert (np.abs(wa - wy) <= 2 * R.gamma(hits) * np.maximum(wa, wy)).all()
    # features, C = 5
    feats = T(np.random.default_rng(2).normal(size=(c.n, 5)))
    fa = _call(c, True, features=feats)[0][-1]
    fy = _call(c, False, opacities=comp_op, features=feats)[0][-1]
    assert fa.shape[0] == 5 and torch.equal(fa, fy)
    # a two-band partition composes to the frame (one tile row: the frame is its own band)
    gy = (c.h + 15) // 16
    if gy >= 2:
        bands = [_call(c, True, tile_rows=(0, 1))[0], _call(c, True, tile_rows=(1, gy - 1))[0]]
        for k in [0] + ([2, 3] if c.aux else []):
            assert torch.equal(bands[0][k] + bands[1][k], out_a[k]), f'output {k}: the bands do not compose to the frame'
        assert torch.equal(bands[0][1], out_a[1]) and torch.equal(bands[1][1], out_a[1])


# ------------------------------------------------------------------------------------------------------------------------ 2. the compensated opacity
def _opacity64(c):
    return AA.sigmoid64(c.sc['raw']['logit'][:, 0]) if c.form == 'raw' else np.asarray(c.sc['opacities'], f64)


@pytest.mark.parametrize('name', list(CASES))
def test_2_compensated_opacity_within_its_budget(name):
    c = _case(name)
    _, _, st, _ = _call(c, True)
    vis = st['radii'].reshape(-1)[:c.n] > 0
    q = AA.comp64(c.sc['means3D'], st['cov3D'].reshape(-1, 6)[:c.n], c.cam)
    floor = AA.classify(q, vis)
    o = _opacity64(c)
    got = _compensated(st, c.n).astype(f64)
    want = o * q.comp
    budget = o * q.b_comp + R.gamma(1 + (AA.C_SIGMOID if c.form == 'raw' else 0)) * want
    err = np.abs(got - want)
    live = vis & ~floor
    print(f'{name}: worst err / budget of o comp {(err[live] / budget[live]).max(initial=0):.3f} over {int(live.sum())} Gaussians, {int(floor.sum())} at the floor')
    assert (err[live] <= budget[live]).all()
    assert (got[~vis] == 0).all()
    if floor.any():     # o * sqrtf(0.000025f) to 1 ulp
        o32 = np.asarray(c.sc['opacities'], np.float32)[floor]
        f = o32 * np.sqrt(np.float32(0.000025))
        assert (np.abs(got[floor] - f.astype(f64)) <= np.spacing(f).astype(f64)).all()


# ------------------------------------------------------------------------------------------------------------------------ 3. backward
def _reference(c, st_kernel, comp_op):
    """The judged reference of the blend on the kernel's state (gs_grad_cases.reference on the case with the compensated opacities: the oracle's decisions are
    asserted equal to the kernel's), and comp64 of that state."""
    cy = copy.copy(c)
    cy.sc = dict(c.sc, opacities=comp_op)
    cy.form = 'sh' if c.form == 'raw' else c.form
    st, _ = C.forward(cy)
    _check_state(st, st_kernel)
    r = C.reference(cy, st, kernel_state=_kernel_floats(st, st_kernel))
    q = AA.comp64(c.sc['means3D'], st_kernel['cov3D'].reshape(-1, 6)[:c.n], c.cam)
    return st, r, q


def _backward(c, out, r):
    if c.aux:
        torch.autograd.backward([out[0], out[2], out[3]], [T(r.g), T(r.g_d), T(r.g_a)])
    else:
        out[0].backward(T(r.g))


def _assert_rows_equal(name, got, like, tiles, mag):
    """Bit-equal where at most two tiles deposit (module docstring); the reordering bound elsewhere."""
    exact = tiles <= 2
    np.testing.assert_array_equal(got[exact], like[exact], err_msg=name)
    rest = ~exact
    if rest.any():
        bound = (2 * R.gamma(tiles[rest]))[:, None] * mag[rest]
        assert (np.abs(got[rest].astype(f64) - like[rest].astype(f64)) <= bound).all(), name


@pytest.mark.parametrize('name', list(CASES))
def test_3_every_gradient_element_within_its_budget(name):
    c = _case(name)
    out, leaves, st_k, _ = _call(c, True, absgrad=True)
    comp_op = _compensated(st_k, c.n)
    st, r, q = _reference(c, st_k, comp_op)
    vis = st.radii > 0
    floor = AA.classify(q, vis)
    leaf = AA.aa_leaf_ref(c, r, q, _opacity64(c), vis)
    _backward(c, out, r)
    got = _gradients_of(c, leaves)
    for k, (worst, over, nonzero) in C.judge_all(c, got, leaf, 'antialiased ').items():
        assert over == 0 and nonzero == 0, (name, k, worst, over, nonzero)
    if c.form == 'raw':
        return          # (no yardstick run: test 1's identity is stated for activated parameters)
    # the yardstick run of test 1 with the same pixel gradients
    out_y, leaves_y, _, _ = _call(c, False, opacities=comp_op, absgrad=True)
    _backward(c, out_y, r)
    like = _gradients_of(c, leaves_y)
    tiles = r.ref['tiles']
    A2 = np.concatenate([r.ref['A'][:, 4:6], np.zeros((c.n, 1))], 1)
    _assert_rows_equal('means2D.grad', got['mean2D'], like['mean2D'], tiles, A2)
    # absgrad: its addends are the magnitudes of mean2D's, so A bounds them too
    _assert_rows_equal('means2D.absgrad', leaves['mean2D'].absgrad.cpu().numpy(), leaves_y['mean2D'].absgrad.cpu().numpy(), tiles, A2)
    if floor.any():
        rows = floor & (tiles <= 2)
        assert rows.any()
        for k in C.leaf_names(c):
            if k in ('mean2D', 'opacity'):
                continue
            np.testing.assert_array_equal(got[k][rows], like[k][rows], err_msg=f'{k} of the floor-hitting Gaussians')
        comp32 = np.sqrt(np.float32(0.000025))
        want = like['opacity'].reshape(-1)[rows] * comp32
        assert (np.abs(got['opacity'].reshape(-1)[rows].astype(f64) - want.astype(f64)) <= np.spacing(np.abs(want)).astype(f64)).all()


# ------------------------------------------------------------------------------------------------------------------------ 4. the Python surface
def test_4_settings_field_and_keyword_agree():
    c = _case('p127-40x24-deg3')
    a, _, sa, _ = _call(c, True)
    b, _, sb, _ = _call(c, False, settings_flag=True)
    _assert_same_frame(a, b, sa, sb, 2)
    plain = _call(c, False)
    assert not torch.equal(plain[0][0], a[0])
    # without the flag: a second call gives the same bits
    again = _call(c, False)
    _assert_same_frame(plain[0], again[0], plain[2], again[2], 2)


def test_4_rest_step_and_camera_grad_are_refused():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    from nerficg_amd.gaussian_splatting import render_image_training
    from tests import scenes
    from tests.test_gpu_gs_pose_grad import _gaussians, _perspective
    c = _case('p127-40x24-deg3')
    t = {k: T(v) for k, v in c.sc.items() if k != 'sh_degree'}

    class Step:
        def take(self):
            raise AssertionError('the step must not be taken')

    common = dict(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None], scales=t['scales'], rotations=t['rotations'])
    with pytest.raises(RuntimeError, match='antialiasing together with rest_step'):
        GaussianRasterizer(_settings(c))(shs=t['shs'][:, :1].contiguous(), shs_rest=t['shs'][:, 1:].contiguous(), rest_step=Step(), antialiasing=True, **common)
    rs = _settings(c)
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='antialiasing together with camera_grad'):
        GaussianRasterizer(rs)(shs=t['shs'], camera_grad=True, antialiasing=True, **common)
    with pytest.raises(RuntimeError, match='antialiasing together with camera_grad'):
        GaussianRasterizer(rs._replace(antialiasing=True))(shs=t['shs'], camera_grad=True, **common)
    g = _gaussians(c.sc)
    g.training_setup(training_cameras_extent=3.0)
    cam, c2w = _perspective(c.w, c.h), scenes.orbit_pose(*C.POSE)
    with pytest.raises(RuntimeError, match='antialiasing'):
        render_image_training(g, cam, c2w, fuse_rest_step=True, antialiasing=True)
    g.fuse_rest_step = True                                       # the model's own default: resolves to "not fused" with the flag
    out = render_image_training(g, cam, c2w, antialiasing=True)
    out['rgb'].sum().backward()
    assert g._features_rest.grad is not None and g._opacities.grad is not None
    plain = render_image_training(g, cam, c2w, fuse_rest_step=False)
    assert not torch.equal(plain['rgb'], out['rgb'])


# ------------------------------------------------------------------------------------------------------------------------ 5. the 3-D filter
def _filter_views(V):
    from tests import scenes
    rng = np.random.default_rng(V)
    rows = []
    for v in range(V):
        c2w = scenes.orbit_pose(rng.uniform(0, 6.28), rng.uniform(-0.5, 0.5), rng.uniform(2.0, 4.0))
        fx = float(rng.choice([40.0, 48.0, 64.0]))
        rows.append(AA.view_block(np.linalg.inv(c2w), fx, fx * 1.1, 40, 24))
    return np.stack(rows)


def _filter_points(P, views):
    """Random points around the origin; with P >= 129 also 16 points far outside every frame (seen by no view) and 16 points at the 1.15 border of view 0
    (x / z fx + W / 2 = 1.15 W): the first on it up to the rounding of the transforms, then alternately 0.1 % inside and outside."""
    rng = np.random.default_rng(P)
    p = rng.uniform(-1.0, 1.0, size=(P, 3)).astype(np.float32)
    if P >= 129:
        p[:16] = (rng.normal(size=(16, 3)) * 0.01 + np.array([0.0, 60.0, 0.0])).astype(np.float32)
        c = views[0].astype(f64)
        w2c = c[:16].reshape(4, 4)
        c2w = np.linalg.inv(w2c)
        for j in range(16, 32):
            z = 1.0 + 0.125 * (j - 16)
            side = 1.0 if j == 16 else (1.0 - 1e-3 if j % 2 == 0 else 1.0 + 1e-3)
            cam_pt = np.array([0.65 * c[18] / c[16] * z * side, 0.0, z, 1.0])     # x / z = 0.65 W / fx: the border
            p[j] = (c2w @ cam_pt)[:3].astype(np.float32)
    return p


@pytest.mark.parametrize('P', [1, 129, 1000])
@pytest.mark.parametrize('V', [1, 3, 70])
def test_5_filter3d_against_the_reference(P, V):
    from nerficg_amd.gaussian_splatting import filter_3d
    views = _filter_views(V)
    pts = _filter_points(P, views)
    want, seen = AA.filter3d_ref(pts, views)
    got = filter_3d(T(pts), T(views))
    again = filter_3d(T(pts), T(views))
    assert torch.equal(got, again)
    g = got.cpu().numpy()
    w32 = want.astype(np.float32)
    assert (np.abs(g.astype(f64) - want) <= 2 * np.spacing(w32).astype(f64)).all()
    if P >= 129:
        assert (~seen[:16]).all() and seen.any() and (g[:16] == g[seen].max()).all()      # seen by none: the largest filter among the seen ones
        if V == 1:                                                                         # the border points: inside seen, outside not
            assert seen[18:32:2].all() and not seen[17:32:2].any()


def test_5_filter3d_behind_every_camera():
    from nerficg_amd.gaussian_splatting import filter_3d
    ident = AA.view_block(np.eye(4), 32.0, 32.0, 64, 48)[None]
    pts = np.array([[0, 0, -1.0], [0, 0, 0.19], [0.3, 0.2, -7.0]], np.float32)
    assert (filter_3d(T(pts), T(ident)) == 0).all()                                       # none seen at all: zeros
    pts = np.array([[0, 0, -1.0], [0, 0, 2.0], [2.5, 0, 2.0], [2.7, 0, 2.0]], np.float32)
    want, seen = AA.filter3d_ref(pts, ident)
    assert seen.tolist() == [False, True, True, False]
    np.testing.assert_array_equal(filter_3d(T(pts), T(ident)).cpu().numpy(), want.astype(np.float32))


def test_5_gaussians_carry_the_filter():
    from nerficg_amd.gaussian_splatting import render_image_inference, render_image_training
    from tests import scenes
    from tests.test_gpu_gs_pose_grad import _gaussians, _perspective
    c = _case('p300-40x24-deg3-aux')
    g = _gaussians(c.sc)
    g.training_setup(training_cameras_extent=3.0)
    cam = _perspective(c.w, c.h)
    views = [(cam, scenes.orbit_pose(th, 0.3, 3.0)) for th in (0.5, 2.0, 4.0)]
    assert g.filter_3D is None
    with pytest.raises(RuntimeError, match='compute_3d_filter'):
        g.get_scales_with_3d_filter
    plain = render_image_training(g, *views[0])['rgb']
    f = g.compute_3d_filter(views)
    assert tuple(f.shape) == (c.n, 1) and f.dtype == torch.float32
    block = np.stack([AA.view_block(np.linalg.inv(c2w), cam.focal_x, cam.focal_y, cam.width, cam.height) for _, c2w in views])
    want, _ = AA.filter3d_ref(c.sc['means3D'], block)
    assert (np.abs(f[:, 0].cpu().numpy().astype(f64) - want) <= 2 * np.spacing(want.astype(np.float32)).astype(f64)).all()
    # the two getters against their float64 formulas
    s, o, f64_ = g.get_scales.detach().cpu().numpy().astype(f64), g.get_opacities.detach().cpu().numpy().astype(f64), f.cpu().numpy().astype(f64)
    np.testing.assert_allclose(g.get_scales_with_3d_filter.detach().cpu().numpy(), np.sqrt(s * s + f64_ * f64_), rtol=4 * R.U)
    want_o = o * np.sqrt(np.prod(s * s, 1) / np.prod(s * s + f64_ * f64_, 1))[:, None]
    np.testing.assert_allclose(g.get_opacities_with_3d_filter.detach().cpu().numpy(), want_o, rtol=16 * R.U)
    # rendered through the activated-value path, differentiable to the raw tensors
    out = render_image_training(g, *views[0], antialiasing=True)
    assert not torch.equal(out['rgb'], plain)
    out['rgb'].sum().backward()
    assert g._scales.grad is not None and g._opacities.grad is not None and g._features_rest.grad is not None
    assert render_image_inference(g, *views[0], antialiasing=True)['rgb'].shape == (c.h, c.w, 3)
    # a filter of another length raises; a change of the number of Gaussians drops it
    g.filter_3D = f[:-1]
    with pytest.raises(RuntimeError, match='compute_3d_filter'):
        render_image_training(g, *views[0])
    with pytest.raises(RuntimeError, match='compute_3d_filter'):
        render_image_inference(g, *views[0])
    g.filter_3D = f
    mask = torch.zeros(c.n, dtype=torch.bool, device=DEV)
    mask[::7] = True
    g.prune_points(mask)
    assert g.filter_3D is None
    g.compute_3d_filter(views)
    assert g.filter_3D.shape[0] == g.get_positions.shape[0]
    g.densification_gradient_accum += 1.0
    g.n_observations += 1
    g.percent_dense = 0.01
    g.densify_and_prune(0.0002, 0.005, False)
    assert g.filter_3D is None
