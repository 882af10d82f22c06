"""GPU: gradients of the 3DGS rasterizer to the camera (camera_grad=True; C ABI nrc_gs_backward_pose_band / nrc_gs_camera_block_backward).

Reference: tests/gs_pose_grad_ref.py -- the float64 restatement of the camera chain driven by the CPU oracle's per-Gaussian gradients, held against central
differences in tests/test_gs_pose_grad_ref_cpu.py.  Gate for every camera gradient, per entry: |got - want| <= 2e-3 mag + 1e-6 with mag the sum of the
absolute values of that entry's per-Gaussian addends (each addend is a forward quantity times a per-Gaussian gradient the project holds to 2e-3 of its
tensor's scale); entries whose reference is structurally zero (viewmatrix[:, 3], projmatrix[:, 2], campos with precomputed colours or SH degree 0) must be
exactly zero.

Measured on the MI355X, largest |got - want| / mag over all entries (every test prints its own; the gate is 2e-3):
    test_camera_gradients_match_the_reference   viewmatrix 1.4e-4 (the one-tile frame; 6.7e-5 for 200 000 Gaussians, 1.7e-5 for the single Gaussian, <= 5.8e-6 elsewhere)   projmatrix 3.4e-7   campos 3.1e-6
    precomputed colours / covariances           viewmatrix 1.5e-6   projmatrix 7.1e-8   campos 4.8e-7 (exactly 0 with precomputed colours)
    raw parameters + split SH                   viewmatrix 3.9e-6   projmatrix 1.1e-7   campos 4.6e-7
    depth and alpha maps (all / depth / alpha)  viewmatrix 5.9e-6   projmatrix 1.4e-7   campos 2.9e-6 (exactly 0 without a colour gradient)
    against the kernels' own records            viewmatrix 3.4e-6   projmatrix 1.6e-7   campos 2.7e-6
    band shares against the whole frame         3.8e-8;   translation identity 3.7e-8;   camera block backward 3.8e-8 of the sum of |addends|."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from tests import scenes
from tests.gs_depth_alpha_ref import oracle_pair
from tests.gs_pose_grad_ref import c2w_gradient, c2w_gradient_mag, expected_camera_gradients, oracle_gradients_with_maps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BG = [0.2, 0.4, 0.1]
POSE = (0.5, 0.3, 3.0)
CAMERA = ('viewmatrix', 'projmatrix', 'campos')
REF_NAME = dict(viewmatrix='view', projmatrix='proj', campos='campos')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _settings(cam, deg, needs=(True, True, True), bg=BG):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings
    pose = {k: T(cam[k]).requires_grad_(bool(n)) for k, n in zip(CAMERA, needs)}
    return GaussianRasterizationSettings(
        image_height=cam['height'], image_width=cam['width'], tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=T(np.asarray(bg, np.float32)),
        scale_modifier=1.0, viewmatrix=pose['viewmatrix'], projmatrix=pose['projmatrix'], sh_degree=deg, campos=pose['campos'], prefiltered=False, debug=False)


def _run(sc, cam, camera_grad=True, needs=(True, True, True), **kw):
    """One call of the drop-in module on leaves that require grad.  Returns dict(out, rs, leaves, n_contrib, final_T)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    t = {k: T(v).requires_grad_(True) for k, v in sc.items() if k != 'sh_degree'}
    t['means2D'] = torch.zeros_like(t['means3D'], requires_grad=True)
    rs = _settings(cam, sc['sh_degree'], needs)
    out = GaussianRasterizer(rs)(means3D=t['means3D'], means2D=t['means2D'], opacities=t['opacities'][:, None], shs=t['shs'], scales=t['scales'],
                                 rotations=t['rotations'], camera_grad=camera_grad, **kw)
    st = out[0].grad_fn.debug_state
    return dict(out=out, rs=rs, leaves=t, n_contrib=st['n_contrib'], final_T=st['final_T'])


def _check(got, want, label=''):
    """got: name -> tensor (viewmatrix / projmatrix / campos); want: expected_camera_gradients' dict.  Returns the largest ratio per tensor."""
    ratios = {}
    for name in CAMERA:
        g = got[name]
        ref, mag = want[REF_NAME[name]]
        assert g is not None, name
        gnp = g.detach().cpu().numpy().astype(np.float64)
        assert gnp.shape == ref.shape and np.isfinite(gnp).all(), name
        zero = mag == 0
        assert not gnp[zero].any(), (name, 'an entry whose reference is structurally zero', gnp)
        err = np.abs(gnp - ref)
        ratios[name] = float((err[~zero] / mag[~zero]).max()) if (~zero).any() else 0.0
        print(f'{label}{name}: largest |got - want| / mag = {ratios[name]:.3e} (gate 2e-3), largest |want| = {np.abs(ref).max():.3e}')
        assert np.all(err <= 2e-3 * mag + 1e-6), (name, err, mag)
    return ratios


def _camera_grads(run):
    return {k: getattr(run['rs'], k).grad for k in CAMERA}


def _single(kind):
    """One Gaussian of SH degree 0 at 32 x 32.  'wide': a hand-made splat of sigma ~ 3 pixels around the image centre.  'sub-pixel': the generator's, log-scale mean
    log 0.03, cov2D dominated by the 0.3 low-pass.  The blend backward's conic sums are fixed point (resolution 2^-25 of the tile's largest pixel gradient per
    addition): an absolute error of order 1e-5 for pixel gradients of order 1 (measured 1.1e-5 when this test was written, with a conversion that
    lost 8 bits of a negative sum's low word; tests/test_gpu_gs_grad_budget.py now holds every element to its own budget).  The wide splat's conic gradient is of order 10, so
    that error is 1e-6 of it; the sub-pixel splat's is 0.003 .. 0.03, the error 4e-4 of its largest component and 4e-3 of its smallest -- with a single addend
    per camera entry that IS the entry's relative error, whatever the camera chain does.  The gate against the oracle is therefore asked of the wide splat; the
    sub-pixel one is held against the chain driven by the kernels' own per-Gaussian gradients (test_the_kernel_follows_the_gpu_records)."""
    if kind == 'sub-pixel':
        sc = scenes.gs_random_scene(1, seed=0, extent=1.2, log_scale_mean=math.log(0.03), sh_degree=0)
        return sc, scenes.gs_camera(32, 32, scenes.orbit_pose(0.9, 0.35, 3.2))
    q = np.array([[0.8, 0.3, -0.4, 0.33]], np.float32)
    shs = np.zeros((1, 16, 3), np.float32)
    shs[0, 0] = (0.5, -0.2, 0.8)
    sc = dict(means3D=np.array([[0.1, -0.05, 0.2]], np.float32), scales=np.array([[0.30, 0.18, 0.24]], np.float32), rotations=q / np.linalg.norm(q),
              opacities=np.array([0.7], np.float32), shs=shs, sh_degree=0)
    return sc, scenes.gs_camera(32, 32, scenes.orbit_pose(*POSE))


@functools.lru_cache(maxsize=None)
def _scene(n, w=0, h=0, deg=0, seed=11, pose=POSE, extent=1.0, log_scale=math.log(0.06), behind=0):
    if n == 'single':
        return _single(w)
    sc = scenes.gs_random_scene(n, seed=seed, extent=extent, log_scale_mean=log_scale, sh_degree=deg)
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(*pose))
    if behind:                         # the first `behind` Gaussians mirrored through the camera centre: behind the camera, culled
        sc['means3D'][:behind] = 2 * cam['campos'][None] - sc['means3D'][:behind]
    return sc, cam


@functools.lru_cache(maxsize=None)
def _oracle(key):
    sc, cam = _scene(*key)
    return oracle_pair(sc, cam, BG)


def _pixel_gradient(h, w, seed):
    return np.random.default_rng(seed).normal(size=(3, h, w)).astype(np.float32)


CASES = {
    'scene A': (300, 64, 48, 3),
    'one Gaussian': ('single', 'wide'),
    'P = 127': (127, 64, 48, 3, 5),
    'P = 128': (128, 64, 48, 3, 6),
    'P = 129': (129, 64, 48, 3, 7),
    'many slabs': (5000, 160, 96, 2),
    'one tile': (5000, 16, 16, 2),
    'more chunks than workgroups': (200_000, 160, 96, 3, 13, POSE, 1.0, math.log(0.01)),       # 1563 chunks on at most 1536 workgroups: the grid-stride walk
    'empty chunks': (600, 64, 48, 3, 12, POSE, 1.0, math.log(0.06), 256),
}


# ------------------------------------------------------------------------------------------------------------------------ 1. the gradient exists and is right
@pytest.mark.parametrize('case', list(CASES))
def test_camera_gradients_match_the_reference(case):
    key = CASES[case]
    sc, cam = _scene(*key)
    colour, aux, st, st2 = _oracle(key)
    h, w = cam['height'], cam['width']
    assert (st.radii > 0).sum() >= 1
    if case == 'empty chunks':
        assert not (st.radii[:256] > 0).any() and (st.radii[256:] > 0).sum() > 100
    g = _pixel_gradient(h, w, 3)
    run = _run(sc, cam)
    run['out'][0].backward(T(g))
    want = expected_camera_gradients(sc, cam, st, oracle.gs_backward(st, g))
    _check(_camera_grads(run), want, label=f'{case}: ')
    assert np.abs(want['view'][0]).max() > 0 and np.abs(want['proj'][0]).max() > 0


def test_no_gaussians_give_zero_camera_gradients():
    sc, cam = _scene(300, 64, 48, 3)
    empty = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    run = _run(empty, cam)
    run['out'][0].backward(T(_pixel_gradient(48, 64, 3)))
    for name, g in _camera_grads(run).items():
        assert g is not None and g.shape == getattr(run['rs'], name).shape and not g.any(), name


# ------------------------------------------------------------------------------------------------------------------------ 2. modes
def _precomp_leaves(sc, st, cols=None, cov=False):
    t = dict(means3D=T(sc['means3D']).requires_grad_(True), opacities=T(sc['opacities'])[:, None].requires_grad_(True))
    t['means2D'] = torch.zeros_like(t['means3D'], requires_grad=True)
    kw = dict(means3D=t['means3D'], means2D=t['means2D'], opacities=t['opacities'])
    if cols is not None:
        kw['colors_precomp'] = t['colors'] = T(cols).requires_grad_(True)
    else:
        kw['shs'] = t['shs'] = T(sc['shs']).requires_grad_(True)
    if cov:
        kw['cov3D_precomp'] = t['cov'] = T(st.cov3D).requires_grad_(True)
    else:
        kw['scales'], kw['rotations'] = T(sc['scales']).requires_grad_(True), T(sc['rotations']).requires_grad_(True)
    return t, kw


@pytest.mark.parametrize('colours,cov', [(True, False), (False, True), (True, True)])
def test_precomputed_colours_and_covariances(colours, cov):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    key = CASES['scene A']
    sc, cam = _scene(*key)
    _, _, st_sh, _ = _oracle(key)
    cols = np.random.default_rng(1).random((300, 3)).astype(np.float32) if colours else None
    colour, _, st, _ = oracle_pair(sc, cam, BG, colors_precomp=cols, cov3D_precomp=st_sh.cov3D if cov else None)
    rs = _settings(cam, 3)
    t, kw = _precomp_leaves(sc, st_sh, cols, cov)
    image, radii = GaussianRasterizer(rs)(camera_grad=True, **kw)
    np.testing.assert_allclose(image.detach().cpu().numpy(), colour, rtol=0, atol=2e-5)
    g = _pixel_gradient(48, 64, 4)
    image.backward(T(g))
    want = expected_camera_gradients(sc, cam, st, oracle.gs_backward(st, g))
    got = {k: getattr(rs, k).grad for k in CAMERA}
    _check(got, want, label=f'precomp colours={colours} cov={cov}: ')
    if colours:
        assert not want['campos'][1].any() and not got['campos'].any()          # no SH, no view direction: exactly zero


def test_raw_parameters_with_split_sh():
    """The activations in the kernel's own operation order (as test_gpu_gs_depth_alpha does), so that the oracle sees the geometry the kernels see."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    n, w, h = 1000, 96, 64
    rng = np.random.default_rng(7)
    sc, cam = _scene(n, w, h, 3, 21, (0.4, 0.25, 3.0), 1.0, math.log(0.05))
    logit = T(np.log(sc['opacities'] / (1 - sc['opacities'])).astype(np.float32)[:, None])
    log_scale = T(np.log(sc['scales']).astype(np.float32))
    q = T((sc['rotations'] * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32))
    norm = torch.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]).clamp_min(1e-12)
    act = dict(sc, opacities=(1.0 / (1.0 + torch.exp(-logit)))[:, 0].cpu().numpy(), scales=torch.exp(log_scale).cpu().numpy(), rotations=(q / norm[:, None]).cpu().numpy())
    colour, _, st, _ = oracle_pair(act, cam, BG)
    rs = _settings(cam, 3)
    image, radii = GaussianRasterizer(rs)(means3D=T(sc['means3D']), means2D=torch.zeros(n, 3, device=DEV), opacities=logit, shs=T(sc['shs'][:, :1]),
                                          shs_rest=T(sc['shs'][:, 1:]), scales=log_scale, rotations=q, raw_parameters=True, camera_grad=True)
    np.testing.assert_allclose(image.detach().cpu().numpy(), colour, rtol=0, atol=2e-5)
    assert int((radii > 0).sum()) > 300
    g = _pixel_gradient(h, w, 5)
    image.backward(T(g))
    _check({k: getattr(rs, k).grad for k in CAMERA}, expected_camera_gradients(act, cam, st, oracle.gs_backward(st, g)), label='raw + split SH: ')


def _upstream(h, w, mode, seed):
    rng = np.random.default_rng(seed)
    g_rgb, g_d, g_a = (rng.normal(size=s).astype(np.float32) for s in ((3, h, w), (h, w), (h, w)))
    if mode != 'all':
        g_rgb[:] = 0
        (g_a if mode == 'depth_only' else g_d)[:] = 0
    return g_rgb, g_d, g_a


@pytest.mark.parametrize('mode', ['all', 'depth_only', 'alpha_only'])
def test_with_depth_and_alpha_maps(mode):
    key = CASES['scene A']
    sc, cam = _scene(*key)
    colour, aux, st, st2 = _oracle(key)
    g_rgb, g_d, g_a = _upstream(48, 64, mode, 300)
    run = _run(sc, cam, return_depth_alpha=True)
    image, radii, depth, alpha = run['out']
    torch.autograd.backward([image, depth, alpha], [T(g_rgb), T(g_d), T(g_a)])
    grads, gz = oracle_gradients_with_maps(st, st2, cam, g_rgb, g_d, g_a)
    want = expected_camera_gradients(sc, cam, st, grads, gz=gz)
    _check(_camera_grads(run), want, label=f'maps {mode}: ')
    if mode != 'all':
        assert not want['campos'][1].any() and not _camera_grads(run)['campos'].any()          # no colour gradient: the SH direction receives exactly nothing


@pytest.mark.parametrize('which', [0, 1, 2])
def test_only_one_tensor_requires_grad(which):
    key = CASES['scene A']
    sc, cam = _scene(*key)
    _, _, st, _ = _oracle(key)
    g = _pixel_gradient(48, 64, 3)
    needs = tuple(k == which for k in range(3))
    run = _run(sc, cam, needs=needs)
    run['out'][0].backward(T(g))
    want = expected_camera_gradients(sc, cam, st, oracle.gs_backward(st, g))
    for k, name in enumerate(CAMERA):
        grad = getattr(run['rs'], name).grad
        if k != which:
            assert grad is None, name
            continue
        ref, mag = want[REF_NAME[name]]
        err = np.abs(grad.cpu().numpy().astype(np.float64) - ref)
        assert grad.shape == getattr(run['rs'], name).shape and np.all(err <= 2e-3 * mag + 1e-6) and not grad.cpu().numpy()[mag == 0].any(), name


# ------------------------------------------------------------------------------------------------------------------------ 3. nothing else moves
def _kept_records():
    from nerficg_amd import diff_gaussian_rasterization as dgr
    return dgr._GRAD_RECORDS[(torch.device(DEV, torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream)]


def test_the_flag_changes_nothing_else_and_leaves_the_records_cleared():
    """On a frame of ONE tile, where the blend backward's records are reproducible: each record receives one addition per quantity.  (With several tiles the
    tile sums reach a record as f32 atomics in arrival order, and every gradient derived from the records differs in its last bits from run to run, with or
    without the flag -- two calls without it included.)  5000 Gaussians: 40 slabs, multi-wave combine."""
    key = CASES['one tile']
    sc, cam = _scene(*key)
    g = T(_pixel_gradient(16, 16, 3))
    plain = _run(sc, cam, camera_grad=False)
    plain['out'][0].backward(g)
    assert all(v is None for v in _camera_grads(plain).values())                 # without the flag: today's call, no camera gradient
    flagged = _run(sc, cam)
    assert int((flagged['out'][1] > 0).sum()) > 4000
    flagged['out'][0].backward(g)
    assert all(v is not None and bool(v.any()) for v in _camera_grads(flagged).values())
    assert torch.equal(flagged['out'][0], plain['out'][0]) and torch.equal(flagged['out'][1], plain['out'][1])
    assert torch.equal(flagged['n_contrib'], plain['n_contrib']) and torch.equal(flagged['final_T'], plain['final_T'])
    for name, leaf in flagged['leaves'].items():
        assert leaf.grad is not None and torch.equal(leaf.grad, plain['leaves'][name].grad), name
    kept = _kept_records()
    assert kept[0] == 5000 and not kept[1].any()                                 # the per-Gaussian backward still clears what the camera pass only read


def test_the_flag_leaves_the_forward_and_the_cleared_records_alone_on_many_tiles():
    key = CASES['many slabs']
    sc, cam = _scene(*key)
    g = T(_pixel_gradient(96, 160, 3))
    plain, flagged = _run(sc, cam, camera_grad=False), _run(sc, cam)
    assert torch.equal(flagged['out'][0], plain['out'][0]) and torch.equal(flagged['out'][1], plain['out'][1])
    assert torch.equal(flagged['n_contrib'], plain['n_contrib']) and torch.equal(flagged['final_T'], plain['final_T'])
    flagged['out'][0].backward(g)
    kept = _kept_records()
    assert kept[0] == 5000 and not kept[1].any()


# ------------------------------------------------------------------------------------------------------------------------ 4. determinism
def test_two_backward_passes_give_the_same_bits():
    """The reduction has no atomics and a fixed order (lanes, rows of a workgroup, slabs): the same records give the same bits.  One tile, so that the records
    are the same (see above); 40 slabs."""
    key = CASES['one tile']
    sc, cam = _scene(*key)
    g = T(_pixel_gradient(16, 16, 3))
    grads = []
    for _ in range(2):
        run = _run(sc, cam)
        run['out'][0].backward(g)
        grads.append(_camera_grads(run))
    for name in CAMERA:
        assert bool(grads[0][name].any()) and torch.equal(grads[0][name], grads[1][name]), name


# ------------------------------------------------------------------------------------------------------------------------ 4b. the kernel against its own inputs
@pytest.mark.parametrize('case', ['sub-pixel', 'one Gaussian', 'scene A', 'many slabs'])
def test_the_kernel_follows_the_gpu_records(case, monkeypatch):
    """The float64 chain of the reference driven by the kernels' OWN per-Gaussian gradients (mean2D and mean3D as returned, the conic gradient through the
    dL_dconic output the wrapper leaves NULL): what the camera pass adds to them is its arithmetic and its summation alone.  Same gate; measured 3.7e-7 of mag
    on the sub-pixel Gaussian, whose distance to the ORACLE-driven reference is 5.8e-3 of mag -- all of it the conic record (4e-4 of its largest component)."""
    import ctypes
    from nerficg_amd import _lib
    lib = _lib.load()
    index = [a for _, a in _lib.parse_header()['nrc_gs_backward_pose_band'][1]].index('dL_dconic')
    real, captured = lib.nrc_gs_backward_pose_band, {}

    def with_conic(*args):
        args = list(args)
        captured['conic'] = torch.zeros(max(args[0], 1), 4, device=DEV)
        args[index] = ctypes.c_void_p(captured['conic'].data_ptr())
        return real(*args)

    monkeypatch.setattr(lib, 'nrc_gs_backward_pose_band', with_conic)
    key = ('single', 'sub-pixel') if case == 'sub-pixel' else CASES[case]
    sc, cam = _scene(*key)
    _, _, st, _ = _oracle(key)
    g = _pixel_gradient(cam['height'], cam['width'], 3)
    run = _run(sc, cam)
    run['out'][0].backward(T(g))
    assert torch.equal(run['out'][1].cpu(), torch.from_numpy(st.radii))                    # the oracle's forward state stands for the kernels' (cov3D, visibility)
    own = dict(mean2D=run['leaves']['means2D'].grad.cpu().numpy(), conic=captured['conic'].cpu().numpy(), mean3D=run['leaves']['means3D'].grad.cpu().numpy(),
               color=oracle.gs_backward(st, g)['color'])
    assert np.abs(own['conic']).max() > 0
    _check(_camera_grads(run), expected_camera_gradients(sc, cam, st, own), label=f'{case}, own records: ')


# ------------------------------------------------------------------------------------------------------------------------ 5. bands
def test_the_shares_of_two_bands_sum_to_the_frame():
    key = (300, 64, 80, 3)                                                       # five tile rows: 2 + 3
    sc, cam = _scene(*key)
    _, _, st, _ = _oracle(key)
    g = _pixel_gradient(80, 64, 8)
    want = expected_camera_gradients(sc, cam, st, oracle.gs_backward(st, g))
    whole = _run(sc, cam)
    whole['out'][0].backward(T(g))
    total = {name: torch.zeros_like(v, dtype=torch.float64) for name, v in _camera_grads(whole).items()}
    for band in ((0, 2), (2, 3)):
        part = _run(sc, cam, tile_rows=band)
        part['out'][0].backward(T(g))
        for name, v in _camera_grads(part).items():
            assert bool(v.any()), (band, name)
            total[name] += v.double()
    _check(_camera_grads(whole), want, label='whole frame: ')
    _check(total, want, label='sum of the band shares: ')
    for name in CAMERA:
        mag = want[REF_NAME[name]][1]
        err = np.abs((total[name] - _camera_grads(whole)[name].double()).cpu().numpy())
        print(f'bands against the whole frame, {name}: {float((err[mag > 0] / mag[mag > 0]).max()):.3e}')
        assert np.all(err <= 2e-3 * mag + 1e-6), name


# ------------------------------------------------------------------------------------------------------------------------ 6. translation identity
def _perspective(w, h):
    from nerficg_amd.gaussian_splatting import PerspectiveCamera
    return PerspectiveCamera(w, h, 1.2 * w, 1.2 * w, background_color=torch.tensor(BG, device=DEV))


def test_translation_identity_on_the_gpu_numbers():
    """Moving the camera equals moving every Gaussian the other way: dL/dc2w[:, 3] = -sum_i dL/dmeans3D_i, both sides from the kernels (the sum in float64)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    from nerficg_amd.gaussian_splatting import make_raster_settings
    sc, cam = _scene(*CASES['scene A'])
    c2w = T(scenes.orbit_pose(*POSE)).requires_grad_(True)
    rs = make_raster_settings(_perspective(64, 48), c2w, 3)
    assert rs.viewmatrix.requires_grad and rs.projmatrix.requires_grad and rs.campos.requires_grad
    np.testing.assert_allclose(rs.viewmatrix.detach().cpu().numpy(), cam['viewmatrix'], rtol=0, atol=1e-6)
    t = {k: T(v).requires_grad_(True) for k, v in sc.items() if k != 'sh_degree'}
    image, radii = GaussianRasterizer(rs)(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None], shs=t['shs'],
                                          scales=t['scales'], rotations=t['rotations'], camera_grad=True)
    image.backward(T(_pixel_gradient(48, 64, 3)))
    assert c2w.grad is not None and c2w.grad.shape == (4, 4) and not c2w.grad[3].any()
    got = c2w.grad[:3, 3].double().cpu().numpy()
    per = t['means3D'].grad.double().cpu().numpy()
    ref, mag = -per.sum(0), np.abs(per).sum(0)
    print('translation identity: |c2w.grad[:, 3] + sum means3D.grad| / mag =', np.abs(got - ref) / mag)
    assert np.all(np.abs(got - ref) <= 2e-3 * mag + 1e-6), (got, ref, mag)


# ------------------------------------------------------------------------------------------------------------------------ 7. the camera block's backward alone
@pytest.mark.parametrize('rows', [3, 4])
def test_camera_block_backward_against_the_reference(rows):
    """Each output is at most eight float32 roundings of a sum of at most seven products: 1e-6 of the sum of the absolute values of its addends."""
    from nerficg_amd import _lib
    from nerficg_amd.gaussian_splatting import _projection_transposed
    rng = np.random.default_rng(9)
    c2w = T(scenes.orbit_pose(0.7, -0.2, 2.5)[:rows])
    proj_t = _projection_transposed(_perspective(64, 48), DEV)
    dcam = T(rng.normal(size=35))
    out = torch.full((12,), float('nan'), device=DEV)
    _lib.check(_lib.load().nrc_gs_camera_block_backward(_lib.ptr(c2w), _lib.ptr(proj_t), _lib.ptr(dcam), _lib.ptr(out), _lib.stream_of(out)), 'camera_block_backward')
    d = dcam.double().cpu().numpy()
    args = (c2w.double().cpu().numpy(), proj_t.double().cpu().numpy(), d[:16].reshape(4, 4), d[16:32].reshape(4, 4), d[32:35])
    want, mag = c2w_gradient(*args), c2w_gradient_mag(*args)
    err = np.abs(out.double().cpu().numpy().reshape(3, 4) - want)
    print('camera block backward: largest |got - want| / sum|addends| =', float((err / mag).max()))
    assert np.all(err <= 1e-6 * mag)


# ------------------------------------------------------------------------------------------------------------------------ 8. refusals
def _gaussians(sc):
    from nerficg_amd.gaussian_splatting import Gaussians
    t = {k: T(v) for k, v in sc.items() if k != 'sh_degree'}
    return Gaussians(t['means3D'], torch.log(t['scales']), t['rotations'], torch.logit(t['opacities'].clamp(1e-4, 1 - 1e-4))[:, None],
                     t['shs'][:, :1].contiguous(), t['shs'][:, 1:].contiguous(), sh_degree=sc['sh_degree'])


def test_rest_step_is_refused():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    from nerficg_amd.gaussian_splatting import render_image_training
    sc, cam = _scene(*CASES['scene A'])
    t = {k: T(v) for k, v in sc.items() if k != 'sh_degree'}

    class Step:
        def take(self):
            raise AssertionError('the step must not be taken')

    with pytest.raises(RuntimeError, match='camera_grad.*rest_step'):
        GaussianRasterizer(_settings(cam, 3))(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'][:, None],
                                             shs=t['shs'][:, :1].contiguous(), shs_rest=t['shs'][:, 1:].contiguous(), scales=t['scales'], rotations=t['rotations'],
                                             rest_step=Step(), camera_grad=True)
    c2w = T(scenes.orbit_pose(*POSE)).requires_grad_(True)
    with pytest.raises(RuntimeError, match='camera_grad'):
        render_image_training(_gaussians(sc), _perspective(64, 48), c2w, fuse_rest_step=True)


# ------------------------------------------------------------------------------------------------------------------------ 9. pose recovery
def test_a_camera_pose_is_recovered_through_render_image_training():
    """Scene A frozen, the target rendered at the true pose, the start 0.05 off in translation and 0.0269 rad off in rotation; Adam (lr 2e-3) on a translation and a
    rotation vector for 100 steps.  Fixed conditions: both errors end below half their start, no Gaussian parameter has a .grad.
    Measured on the MI355X: translation error 0.0500 -> 0.0149, rotation error 0.0269 -> 0.0051 (the float64 reference alone, test_gs_pose_grad_ref_cpu.py, ends at
    0.0149 and 0.0051).  Asserted besides the fixed conditions: twice the measured value where that is the tighter bar (rotation: 0.0102; translation: half the start, 0.025)."""
    from nerficg_amd.gaussian_splatting import render_image_training
    from tests.test_gs_pose_grad_ref_cpu import START_DT, START_ROT, pose_from
    sc, _ = _scene(*CASES['scene A'])
    g = _gaussians(sc)
    for p in g.parameters():
        p.requires_grad_(False)
    cam = _perspective(64, 48)
    c2w_true = T(scenes.orbit_pose(*POSE))
    with torch.no_grad():
        target = render_image_training(g, cam, c2w_true)['rgb'].clone()
    dt, rv = T(START_DT).requires_grad_(True), T(START_ROT).requires_grad_(True)
    opt = torch.optim.Adam([dt, rv], lr=2e-3)
    first = last = None
    for _ in range(100):
        opt.zero_grad()
        image = render_image_training(g, cam, pose_from(c2w_true, dt, rv))['rgb']
        last = ((image - target) ** 2).mean()
        first = last.detach() if first is None else first
        last.backward()
        opt.step()
    e_t, e_r = float(dt.detach().norm()), float(rv.detach().norm())
    print(f'translation error {np.linalg.norm(START_DT):.4f} -> {e_t:.4f}   rotation error {np.linalg.norm(START_ROT):.4f} -> {e_r:.4f}   '
          f'loss {float(first):.2e} -> {float(last.detach()):.2e}')
    assert all(p.grad is None for p in g.parameters())
    assert e_t < 0.5 * np.linalg.norm(START_DT) and e_r < 0.5 * np.linalg.norm(START_ROT)
    assert e_t < POSE_BAR_T and e_r < POSE_BAR_R


POSE_BAR_T, POSE_BAR_R = 0.025, 0.0102     # min(half the start, twice the measured value): 0.0500 / 2 (twice the measured 0.0149 is more), 2 x 0.0051
