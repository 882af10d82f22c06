"""GPU: differentiable depth and alpha maps of the 3DGS rasterizer (return_depth_alpha=True; C ABI nrc_gs_bin_render_aux_band / nrc_gs_backward_aux_band).

Reference: the CPU oracle as it stands, run twice (tests/gs_depth_alpha_ref.py, checked on its own in tests/test_gs_depth_alpha_cpu.py).
Tolerances are the project's own: alpha = 1 - final_T within 2e-6 (the final_T gate of test_gpu_gs_parity.py), depth within the 2e-5 colour gate times
the largest visible depth (the channel's magnitude), every gradient tensor within max error <= 2e-3 scale + 1e-6 and mean error <= 1e-4 scale + 1e-7 of
the oracle (test_backward_matches_oracle), scale = the reference tensor's largest magnitude.  The colour, radii, n_contrib and final_T of a call with
the flag are compared with torch.equal against the call without it."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import scenes
from tests.gs_depth_alpha_ref import expected_gradients, oracle_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BG = [0.2, 0.4, 0.1]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _settings(cam, bg=BG, sh_degree=3):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=cam['height'], image_width=cam['width'], tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=T(np.asarray(bg, np.float32)),
        scale_modifier=1.0, viewmatrix=T(cam['viewmatrix']), projmatrix=T(cam['projmatrix']), sh_degree=sh_degree, campos=T(cam['campos']),
        prefiltered=False, debug=False)


def _run(sc, cam, flag=True, tile_rows=None, bg=BG):
    """One call of the drop-in module on leaves that require grad.  Returns dict(color, radii, depth, alpha, leaves, state)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    t = {k: T(v).requires_grad_(True) for k, v in sc.items() if k != 'sh_degree'}
    t['means2D'] = torch.zeros_like(t['means3D'], requires_grad=True)
    kw = {}
    if tile_rows is not None:
        kw['tile_rows'] = tile_rows
    if flag:
        kw['return_depth_alpha'] = True
    out = GaussianRasterizer(_settings(cam, bg, sc['sh_degree']))(means3D=t['means3D'], means2D=t['means2D'], opacities=t['opacities'][:, None], shs=t['shs'],
                                                                  scales=t['scales'], rotations=t['rotations'], **kw)
    assert len(out) == (4 if flag else 2)
    st = out[0].grad_fn.debug_state
    return dict(color=out[0], radii=out[1], depth=out[2] if flag else None, alpha=out[3] if flag else None, leaves=t,
                n_contrib=st['n_contrib'], final_T=st['final_T'])


@functools.lru_cache(maxsize=None)
def _case(n, w, h, deg, seed, scene_seed, extent, log_scale, pose):
    sc = scenes.gs_random_scene(n, seed=scene_seed, extent=extent, log_scale_mean=log_scale, sh_degree=deg)
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(*pose))
    return (sc, cam) + oracle_pair(sc, cam, BG)


def _check_forward(got, aux, st, h, w):
    vis = st.radii > 0
    zmax = float(np.abs(st.depths[vis]).max()) if vis.any() else 1.0
    assert got['depth'].shape == got['alpha'].shape == (h, w) and got['depth'].dtype == got['alpha'].dtype == torch.float32
    a_err = np.abs(got['alpha'].detach().cpu().numpy() - aux[1]).max()
    d_err = np.abs(got['depth'].detach().cpu().numpy() - aux[0]).max()
    print(f'alpha max error {a_err:.3e} (bound 2e-6)   depth max error {d_err:.3e} (bound {2e-5 * zmax:.3e}, z_max {zmax:.3f})')
    assert a_err <= 2e-6
    assert d_err <= 2e-5 * zmax


def _check_same_as_plain(got, plain):
    for name in ('color', 'radii', 'n_contrib', 'final_T'):
        assert torch.equal(got[name].detach(), plain[name].detach()), f'{name} differs from the call without return_depth_alpha'


GRAD_PAIRS = (('mean3D', 'means3D'), ('mean2D', 'means2D'), ('opacity', 'opacities'), ('scale', 'scales'), ('rot', 'rotations'), ('sh', 'shs'))


def _check_grads(leaves, want, names=GRAD_PAIRS, label=''):
    for ref_name, leaf in names:
        r = want[ref_name]
        g = leaves[leaf].grad
        assert g is not None, leaf
        gnp = g.cpu().numpy().reshape(r.shape)
        assert np.isfinite(gnp).all(), ref_name
        scale = np.abs(r).max()
        if scale == 0:                                   # (SH when no colour gradient is given: exactly nothing arrives)
            assert not gnp.any(), ref_name
            continue
        err = np.abs(gnp - r)
        print(f'{label}{ref_name}: max error {err.max():.3e} (bound {2e-3 * scale + 1e-6:.3e})  mean error {err.mean():.3e} (bound {1e-4 * scale + 1e-7:.3e})')
        assert err.max() <= 2e-3 * scale + 1e-6, (ref_name, err.max(), scale)
        assert err.mean() <= 1e-4 * scale + 1e-7, (ref_name, err.mean(), scale)


def _upstream(h, w, mode, seed):
    rng = np.random.default_rng(seed)
    g_rgb, g_d, g_a = (rng.normal(size=s).astype(np.float32) for s in ((3, h, w), (h, w), (h, w)))
    if mode != 'all':
        g_rgb[:] = 0
        (g_a if mode == 'depth_only' else g_d)[:] = 0
    return g_rgb, g_d, g_a


def _backward(got, g_rgb, g_d, g_a):
    torch.autograd.backward([got['color'], got['depth'], got['alpha']], [T(g_rgb), T(g_d), T(g_a)])


# ------------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('n,w,h,deg,seed', [(1, 32, 32, 0, 0), (500, 100, 70, 3, 1), (20000, 257, 131, 3, 2), (3000, 64, 48, 1, 3)])
def test_forward_maps_match_the_oracle_and_leave_the_colour_alone(n, w, h, deg, seed):
    sc, cam, colour, aux, st, st2 = _case(n, w, h, deg, seed, seed, 1.2, math.log(0.03), (0.9 + seed, 0.35, 3.2))
    assert (st.radii > 0).sum() > 0
    got, plain = _run(sc, cam), _run(sc, cam, flag=False)
    _check_forward(got, aux, st, h, w)
    _check_same_as_plain(got, plain)
    np.testing.assert_allclose(got['color'].detach().cpu().numpy(), colour, rtol=0, atol=2e-5)


# ------------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('mode', ['all', 'depth_only', 'alpha_only'])
@pytest.mark.parametrize('n,w,h,deg', [(300, 64, 48, 3), (5000, 160, 96, 2)])
def test_backward_matches_the_two_oracle_passes(n, w, h, deg, mode):
    """'depth_only' / 'alpha_only': no colour gradient at all -- the tile's early return and its fixed-point exponent must look at the extra channels."""
    sc, cam, colour, aux, st, st2 = _case(n, w, h, deg, 0, 11, 1.0, math.log(0.06), (0.5, 0.3, 3.0))
    g_rgb, g_d, g_a = _upstream(h, w, mode, n)
    got = _run(sc, cam)
    _backward(got, g_rgb, g_d, g_a)
    want = expected_gradients(st, st2, cam, g_rgb, g_d, g_a)
    assert np.abs(want['mean3D']).max() > 0 and np.abs(want['opacity']).max() > 0
    _check_grads(got['leaves'], want, label=f'{mode} ')


def test_a_missing_output_gradient_counts_as_zero():
    sc, cam, colour, aux, st, st2 = _case(300, 64, 48, 3, 0, 11, 1.0, math.log(0.06), (0.5, 0.3, 3.0))
    g_rgb, g_d, g_a = _upstream(48, 64, 'depth_only', 3)
    got = _run(sc, cam)
    got['depth'].backward(T(g_d))                                   # neither the colour nor the alpha map takes part
    _check_grads(got['leaves'], expected_gradients(st, st2, cam, g_rgb, g_d, g_a))


# ------------------------------------------------------------------------------------------------------------------------ more than one batch
def _dense_scene():
    """Many faint, wide splats on a few tiles: tile lists of more than two 256-entry batches, pixels that blend more than 256 of them before they saturate."""
    n = 1500
    sc = scenes.gs_random_scene(n, seed=4, extent=0.3, log_scale_mean=math.log(0.2), sh_degree=1)
    sc['opacities'] = np.full(n, 0.02, np.float32)
    cam = scenes.gs_camera(40, 40, scenes.orbit_pose(0.5, 0.3, 3.0))
    return sc, cam


def test_lists_longer_than_two_batches_forward_and_backward():
    sc, cam = _dense_scene()
    colour, aux, st, st2 = oracle_pair(sc, cam, BG)
    assert int((st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0]).max()) > 512            # more than two batches of both blend kernels
    assert int(st.n_contrib.max()) > 256                                                   # some pixel walks past the first batch
    got, plain = _run(sc, cam), _run(sc, cam, flag=False)
    _check_forward(got, aux, st, 40, 40)
    _check_same_as_plain(got, plain)
    g_rgb, g_d, g_a = _upstream(40, 40, 'all', 9)
    _backward(got, g_rgb, g_d, g_a)
    _check_grads(got['leaves'], expected_gradients(st, st2, cam, g_rgb, g_d, g_a))


# ------------------------------------------------------------------------------------------------------------------------ far depths
@pytest.mark.parametrize('mode', ['all', 'depth_only'])
def test_far_depths_do_not_saturate_the_fixed_point_sums(mode):
    """The backward scene 50 units from the camera, the focal length scaled so that the splats keep their pixel size: z is 50, not of order 1, and the
    depth channel's part of dL/dalpha carries that factor.  A saturated sum is a gradient far outside the bounds (the clamp sits at 2^61 steps)."""
    n, w, h = 300, 64, 48
    sc = scenes.gs_random_scene(n, seed=11, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=3)
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(0.5, 0.3, 50.0), fx=1.2 * w * 50.0 / 3.0)
    colour, aux, st, st2 = oracle_pair(sc, cam, BG)
    vis = st.radii > 0
    assert vis.sum() > 100 and st.depths[vis].min() > 48.0
    got = _run(sc, cam)
    _check_forward(got, aux, st, h, w)
    g_rgb, g_d, g_a = _upstream(h, w, mode, 21)
    _backward(got, g_rgb, g_d, g_a)
    _check_grads(got['leaves'], expected_gradients(st, st2, cam, g_rgb, g_d, g_a), label=f'far {mode} ')


# ------------------------------------------------------------------------------------------------------------------------ parameter forms
def _close(a, b, name):
    scale = float(a.abs().max())
    assert scale > 0 and float((a - b).abs().max()) <= 2e-3 * scale, (name, float((a - b).abs().max()) / max(scale, 1e-30))


def test_raw_parameters_and_split_sh_against_the_activated_call():
    """As test_raw_parameters_and_split_sh_match_the_activated_call, with the two maps.  The activations are written in the kernel's own operation order
    (Model.py:45-87: 1 / (1 + exp(-x)), exp, q / max(|q|, 1e-12) with the squares added left to right), so both calls see the same geometry."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    n, w, h = 6000, 176, 112
    rng = np.random.default_rng(7)
    sc = scenes.gs_random_scene(n, seed=21, extent=1.0, log_scale_mean=np.log(0.05))
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(0.4, 0.25, 3.0))
    rast = GaussianRasterizer(_settings(cam, [0.1, 0.2, 0.3]))
    raw = dict(means3D=sc['means3D'], dc=sc['shs'][:, :1].copy(), rest=sc['shs'][:, 1:].copy(), logit=np.log(sc['opacities'] / (1 - sc['opacities'])).astype(np.float32)[:, None],
               log_scale=np.log(sc['scales']).astype(np.float32), quat=(sc['rotations'] * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32))
    grads = [T(rng.normal(size=s).astype(np.float32)) for s in ((3, h, w), (h, w), (h, w))]
    out = {}
    for mode in ('activated', 'raw'):
        t = {k: T(v).requires_grad_(True) for k, v in raw.items()}
        m2d = torch.zeros(n, 3, device=DEV, requires_grad=True)
        if mode == 'activated':
            q = t['quat']
            norm = torch.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]).clamp_min(1e-12)
            res = rast(means3D=t['means3D'], means2D=m2d, opacities=1.0 / (1.0 + torch.exp(-t['logit'])), shs=torch.cat((t['dc'], t['rest']), dim=1),
                       scales=torch.exp(t['log_scale']), rotations=q / norm[:, None], return_depth_alpha=True)
        else:
            res = rast(means3D=t['means3D'], means2D=m2d, opacities=t['logit'], shs=t['dc'], shs_rest=t['rest'], scales=t['log_scale'],
                       rotations=t['quat'], raw_parameters=True, return_depth_alpha=True)
        torch.autograd.backward([res[0], res[2], res[3]], grads)
        out[mode] = (res, {k: v.grad for k, v in t.items()}, m2d.grad)
    a, b = out['activated'], out['raw']
    assert int((b[0][1] > 0).sum()) > 1000
    assert torch.equal(a[0][2], b[0][2]) and torch.equal(a[0][3], b[0][3]), 'depth and alpha of the raw call differ from the activated call'
    for k in raw:
        _close(a[1][k], b[1][k], k)
    _close(a[2], b[2], 'means2D')


def test_precomputed_colours_and_covariances_against_the_computed_call():
    """Depth and alpha do not depend on the colour source, and the oracle's cov3D is the kernels' own, bit for bit (test_forward_internal_state_matches_oracle):
    the precomputed call must reproduce the maps of the computed call exactly; its gradients are held against the oracle as the existing precomp test does."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    n, w, h = 2000, 96, 80
    sc = scenes.gs_random_scene(n, seed=21, extent=1.0, log_scale_mean=np.log(0.05))
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(2.0, 0.2, 3.0))
    computed = _run(sc, cam, bg=[0, 0, 0])
    _, _, st_sh, _ = oracle_pair(sc, cam, [0, 0, 0])
    cols = np.random.default_rng(1).random((n, 3)).astype(np.float32)
    cov, colp, op, m3 = T(st_sh.cov3D).requires_grad_(True), T(cols).requires_grad_(True), T(sc['opacities'])[:, None].requires_grad_(True), T(sc['means3D']).requires_grad_(True)
    m2d = torch.zeros(n, 3, device=DEV, requires_grad=True)
    color, radii, depth, alpha = GaussianRasterizer(_settings(cam, [0, 0, 0]))(means3D=m3, means2D=m2d, opacities=op, colors_precomp=colp, cov3D_precomp=cov,
                                                                              return_depth_alpha=True)
    assert torch.equal(radii, computed['radii']) and torch.equal(depth, computed['depth']) and torch.equal(alpha, computed['alpha'])
    colour_o, aux, st, st2 = oracle_pair(sc, cam, [0, 0, 0], colors_precomp=cols, cov3D_precomp=st_sh.cov3D)
    np.testing.assert_allclose(color.detach().cpu().numpy(), colour_o, rtol=0, atol=2e-5)
    g_rgb, g_d, g_a = _upstream(h, w, 'all', 2)
    torch.autograd.backward([color, depth, alpha], [T(g_rgb), T(g_d), T(g_a)])
    want = expected_gradients(st, st2, cam, g_rgb, g_d, g_a)
    np.testing.assert_allclose(colp.grad.cpu().numpy(), want['color'], rtol=0, atol=2e-3 * np.abs(want['color']).max())
    np.testing.assert_allclose(cov.grad.cpu().numpy(), want['cov3D'], rtol=0, atol=2e-3 * np.abs(want['cov3D']).max())
    _check_grads(dict(means3D=m3, means2D=m2d, opacities=op), want, names=GRAD_PAIRS[:3], label='precomp ')


# ------------------------------------------------------------------------------------------------------------------------ bands
def test_two_bands_compose_the_maps_and_share_the_gradient():
    n, w, h = 500, 100, 70                       # 5 tile rows, the last one 6 pixel rows high: 2 + 3
    sc, cam, colour, aux, st, st2 = _case(n, w, h, 3, 1, 1, 1.2, math.log(0.03), (1.9, 0.35, 3.2))
    g = _upstream(h, w, 'all', 5)
    whole = _run(sc, cam)
    _backward(whole, *g)
    total = {leaf: torch.zeros_like(whole['leaves'][leaf]) for _, leaf in GRAD_PAIRS}
    depth, alpha = torch.zeros_like(whole['depth']), torch.zeros_like(whole['alpha'])
    for band in ((0, 2), (2, 3)):
        y0, y1 = min(h, 16 * band[0]), min(h, 16 * (band[0] + band[1]))
        part = _run(sc, cam, tile_rows=band)
        for name in ('depth', 'alpha'):
            assert torch.equal(part[name][y0:y1], whole[name][y0:y1]), (band, name)
            assert not part[name][:y0].any() and not part[name][y1:].any(), f'{name}: rows outside the band {band} are touched'
        assert torch.equal(part['color'][:, y0:y1], whole['color'][:, y0:y1])
        depth += part['depth'].detach(); alpha += part['alpha'].detach()
        _backward(part, *g)
        for _, leaf in GRAD_PAIRS:
            total[leaf] += part['leaves'][leaf].grad
    assert torch.equal(depth, whole['depth']) and torch.equal(alpha, whole['alpha'])
    for ref_name, leaf in GRAD_PAIRS:
        r, s = whole['leaves'][leaf].grad, total[leaf]
        scale = float(r.abs().max())
        err = (s - r).abs()
        assert scale > 0 and float(err.max()) <= 2e-3 * scale + 1e-6 and float(err.mean()) <= 1e-4 * scale + 1e-7, (leaf, float(err.max()), scale)
    _check_grads({leaf: type('G', (), {'grad': total[leaf]}) for _, leaf in GRAD_PAIRS}, expected_gradients(st, st2, cam, *g), label='bands ')


# ------------------------------------------------------------------------------------------------------------------------ errors and defaults
def test_rest_step_is_refused_and_the_default_call_is_a_pair():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer, fixed_capacity
    sc, cam, colour, aux, st, st2 = _case(500, 100, 70, 3, 1, 1, 1.2, math.log(0.03), (1.9, 0.35, 3.2))
    t = {k: T(v) for k, v in sc.items() if k != 'sh_degree'}
    rast = GaussianRasterizer(_settings(cam))

    class Step:
        def take(self):
            raise AssertionError('the step must not be taken')

    with pytest.raises(RuntimeError, match='return_depth_alpha.*rest_step'):
        rast(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None], shs=t['shs'][:, :1].contiguous(),
             shs_rest=t['shs'][:, 1:].contiguous(), scales=t['scales'], rotations=t['rotations'], rest_step=Step(), return_depth_alpha=True)
    out = rast(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None], shs=t['shs'], scales=t['scales'], rotations=t['rotations'])
    assert isinstance(out, tuple) and len(out) == 2
    whole = _run(sc, cam)
    with fixed_capacity(st.num_rendered + 1024, 0):               # a capacity that drops nothing: the same maps
        capped = _run(sc, cam)
    assert torch.equal(capped['depth'], whole['depth']) and torch.equal(capped['alpha'], whole['alpha'])


# ------------------------------------------------------------------------------------------------------------------------ the renderer mirror
def test_renderer_mirror_returns_depth_and_alpha_and_trains_through_them():
    from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera, render_image_inference, render_image_training
    W, H = 100, 70
    cam = PerspectiveCamera(W, H, 1.2 * W, 1.2 * W, background_color=torch.tensor([0.1, 0.2, 0.3], device=DEV))
    pose = scenes.orbit_pose(0.4, 0.3, 3.0)
    sc = scenes.gs_random_scene(2000, seed=1, extent=1.0, log_scale_mean=np.log(0.05))
    t = {k: T(v) for k, v in sc.items() if k != 'sh_degree'}
    g = Gaussians(t['means3D'], torch.log(t['scales']), t['rotations'], torch.logit(t['opacities'].clamp(1e-4, 1 - 1e-4))[:, None],
                  t['shs'][:, :1].contiguous(), t['shs'][:, 1:].contiguous())
    plain = render_image_inference(g, cam, pose)
    assert set(plain) == {'rgb'}
    for to_chw, shape in ((False, (H, W, 1)), (True, (1, H, W))):
        out = render_image_inference(g, cam, pose, to_chw=to_chw, depth_alpha=True)
        assert out['alpha'].shape == out['depth'].shape == shape and out['rgb'].shape == ((3, H, W) if to_chw else (H, W, 3))
        assert bool(torch.isfinite(out['alpha']).all()) and bool(torch.isfinite(out['depth']).all())
        assert torch.equal(out['rgb'], render_image_inference(g, cam, pose, to_chw=to_chw)['rgb'])
    g.training_setup(training_cameras_extent=3.0)
    tr = render_image_training(g, cam, pose, depth_alpha=True)
    assert tr['alpha'].shape == tr['depth'].shape == (1, H, W)
    final_T = tr['rgb'].grad_fn.debug_state['final_T'].view(H, W)
    assert torch.equal(tr['alpha'][0].detach(), 1.0 - final_T)                               # 'alpha' is 1 - T of the rasterizer call
    covered = tr['alpha'][0].detach() > 0.5
    z = tr['depth'][0].detach()[covered]
    assert covered.any() and float(z.min()) > 1.0 and float(z.max()) < 5.0                   # normalised: a depth in the scene (orbit radius 3, extent 1)
    (tr['rgb'].mean() + tr['depth'].mean() + tr['alpha'].mean()).backward()
    for name in ('_positions', '_features_dc', '_features_rest', '_opacities', '_scales', '_rotations'):
        grad = getattr(g, name).grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any()), name
    with pytest.raises(RuntimeError, match='depth_alpha'):
        render_image_training(g, cam, pose, fuse_rest_step=True, depth_alpha=True)
