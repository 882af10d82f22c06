"""CPU: the camera gradient of the 3DGS rasterizer -- the float64 reference the GPU tests rely on (tests/gs_pose_grad_ref.py), held against central
differences of oracle.gs_forward(dtype=float64) over all 35 camera entries, with and without depth and alpha gradients; the translation identity (moving the
camera equals moving every Gaussian the other way); the chain back to c2w against torch float64 autograd; the C ABI of the three new entry points (argument
checks run before any HIP call: no GPU needed); and a pose recovered by Adam on the reference alone.

Scene A: 300 Gaussians (seed 11, extent 1, log-scale mean log 0.06, SH degree 3), 64 x 48 from orbit_pose(0.5, 0.3, 3.0), background (0.2, 0.4, 0.1).
Steps of the central differences: 1e-6 and 1e-7 only -- with 1e-5 and more the forward crosses cull and alpha-threshold decisions of this scene and the
quotient is off by a multiple of the derivative."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from nerficg_amd import _lib
from tests import scenes
from tests.gs_depth_alpha_ref import oracle_pair
from tests.gs_pose_grad_ref import c2w_gradient, c2w_gradient_mag, expected_camera_gradients, fov_clamped, oracle_gradients_with_maps

NRC_OK, NRC_ERR_INVALID = 0, -1
W, H, N = 64, 48, 300
BG = [0.2, 0.4, 0.1]
POSE = (0.5, 0.3, 3.0)
SYMBOLS = ('nrc_gs_pose_partials_floats', 'nrc_gs_backward_pose_band', 'nrc_gs_camera_block_backward')


def _f64(d):
    return {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _scene_a():
    sc = scenes.gs_random_scene(N, seed=11, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=3)
    cam = scenes.gs_camera(W, H, scenes.orbit_pose(*POSE))
    return _f64(sc), _f64(cam)


def _forward(sc, cam, dtype=np.float64):
    return oracle.gs_forward(sc['means3D'], sc['opacities'], cam['viewmatrix'], cam['projmatrix'], cam['campos'], cam['tanfovx'], cam['tanfovy'], cam['width'],
                             cam['height'], np.asarray(BG, dtype), sh_degree=sc['sh_degree'], shs=sc['shs'], scales=sc['scales'], rotations=sc['rotations'], dtype=dtype)


ENTRIES = [('viewmatrix', 'view', (k, j)) for k in range(4) for j in range(4)] + [('projmatrix', 'proj', (k, c)) for k in range(4) for c in range(4)] + \
          [('campos', 'campos', (k,)) for k in range(3)]


def _central_differences(value, cam, h):
    out = {}
    for key, name, idx in ENTRIES:
        vals = []
        for sign in (+1.0, -1.0):
            pert = dict(cam)
            pert[key] = cam[key].copy()
            pert[key][idx] += sign * h
            vals.append(value(pert))
        out[(name, idx)] = (vals[0] - vals[1]) / (2 * h)
    return out


def _compare(want, value, cam, label):
    worst = {}
    for h in (1e-6, 1e-7):
        fd = _central_differences(value, cam, h)
        for (name, idx), d in fd.items():
            grad, mag = want[name]
            err = abs(d - grad[idx])
            if mag[idx] == 0:                       # entries the rasterizer does not read: viewmatrix[:, 3], projmatrix[:, 2]
                assert d == 0 and grad[idx] == 0, (name, idx, d, grad[idx])
                continue
            worst[(name, h)] = max(worst.get((name, h), 0.0), err / mag[idx])
            assert err <= 1e-6 * mag[idx], (label, name, idx, h, d, grad[idx], mag[idx])
    print(label, {k: f'{v:.2e}' for k, v in worst.items()}, '(|error| / mag, bound 1e-6)')


def test_a_reference_equals_central_differences_on_all_35_entries():
    sc, cam = _scene_a()
    g = np.random.default_rng(3).normal(size=(3, H, W))
    _, _, st = _forward(sc, cam)
    assert (st.radii > 0).sum() == 297
    assert not fov_clamped(sc, cam, st).any()                      # no visible Gaussian sits on the kink of the 1.3 tan rule
    assert int(st.clamped[st.radii > 0].sum()) == 2               # two colour channels are clamped at zero
    want = expected_camera_gradients(sc, cam, st, oracle.gs_backward(st, g))
    assert all(np.abs(want[k][0]).max() > 0 for k in ('view', 'proj', 'campos'))
    assert not want['view'][0][:, 3].any() and not want['proj'][0][:, 2].any()
    _compare(want, lambda c: float((_forward(sc, c)[0] * g).sum()), cam, 'colour')


def test_b_reference_with_depth_and_alpha_gradients():
    sc, cam = _scene_a()
    rng = np.random.default_rng(4)
    g_rgb, g_d, g_a = rng.normal(size=(3, H, W)), rng.normal(size=(H, W)), rng.normal(size=(H, W))
    _, _, st, st2 = oracle_pair(sc, cam, BG, dtype=np.float64)
    assert not fov_clamped(sc, cam, st).any()
    grads, gz = oracle_gradients_with_maps(st, st2, cam, g_rgb, g_d, g_a)
    assert np.abs(gz).max() > 0
    want = expected_camera_gradients(sc, cam, st, grads, gz=gz)

    def value(c):
        colour, aux, _, _ = oracle_pair(sc, c, BG, dtype=np.float64)
        return float((colour * g_rgb).sum() + (aux[0] * g_d).sum() + (aux[1] * g_a).sum())

    _compare(want, value, cam, 'colour + depth + alpha')


def _proj_t(cam_np):
    """P^T with projmatrix = viewmatrix @ P^T (scenes.gs_camera's P, float32 values)."""
    w, h = cam_np['width'], cam_np['height']
    fx, fy = w / (2 * cam_np['tanfovx']), h / (2 * cam_np['tanfovy'])
    near, far = 0.01, 100.0
    P = np.array([[fx / (w * 0.5), 0.0, 0.0, 0.0], [0.0, fy / (h * 0.5), 0.0, 0.0], [0.0, 0.0, (far + near) / (far - near), -2.0 * far * near / (far - near)],
                  [0.0, 0.0, 1.0, 0.0]], dtype=np.float32)
    return P.T.astype(np.float64)


def test_c_translation_identity():
    """Moving the camera by d equals moving every Gaussian by -d: the last column of dL/dc2w is -sum_i dL/dmean3D_i."""
    sc, cam = _scene_a()
    g = np.random.default_rng(3).normal(size=(3, H, W))
    c2w = scenes.orbit_pose(*POSE)
    proj_t = _proj_t(cam)
    # the camera exactly as c2w builds it, in float64 (scenes.gs_camera rounds to float32: a camera 6e-8 beside the one c2w_gradient differentiates)
    view = np.eye(4)
    view[:3, :3], view[3, :3] = c2w[:3, :3], -(c2w[:3, :3].T @ c2w[:3, 3])
    cam = dict(cam, viewmatrix=view, projmatrix=view @ proj_t, campos=c2w[:3, 3].copy())
    _, _, st = _forward(sc, cam)
    assert (st.radii > 0).sum() == 297
    grads = oracle.gs_backward(st, g)
    want = expected_camera_gradients(sc, cam, st, grads)
    got = c2w_gradient(c2w, proj_t, want['view'][0], want['proj'][0], want['campos'][0])[:, 3]
    ref = -grads['mean3D'].sum(0)
    mag = np.abs(grads['mean3D']).sum(0)
    print('translation identity: |error| / mag', np.abs(got - ref) / mag)
    assert np.all(np.abs(got - ref) <= 1e-9 * mag), (got, ref, mag)


def test_d_c2w_gradient_against_torch_autograd():
    rng = np.random.default_rng(8)
    c2w = scenes.orbit_pose(0.7, -0.2, 2.5)
    proj_t = _proj_t(scenes.gs_camera(W, H, c2w))
    dview, dproj, dcampos = rng.normal(size=(4, 4)), rng.normal(size=(4, 4)), rng.normal(size=3)
    pose = torch.tensor(c2w, dtype=torch.float64, requires_grad=True)
    # the tensor-op camera of gaussian_splatting.make_raster_settings (its branch for a tensor that is not on the GPU), in float64
    rot, pos = pose[:3, :3], pose[:3, 3]
    last_row = torch.cat([-(rot.T @ pos), pose.new_ones(1)])
    view = torch.cat([torch.cat([rot, pose.new_zeros(3, 1)], dim=1), last_row[None]], dim=0)
    proj = view @ torch.tensor(proj_t)
    (view * torch.tensor(dview)).sum().add((proj * torch.tensor(dproj)).sum()).add((pos * torch.tensor(dcampos)).sum()).backward()
    got = c2w_gradient(c2w, proj_t, dview, dproj, dcampos)
    mag = c2w_gradient_mag(c2w, proj_t, dview, dproj, dcampos)
    assert np.all(np.abs(got - pose.grad.numpy()[:3]) <= 1e-14 * mag)
    assert not pose.grad.numpy()[3].any()
    # and that branch itself, float32 on the CPU, builds this camera
    from nerficg_amd.gaussian_splatting import PerspectiveCamera, make_raster_settings
    pc = PerspectiveCamera(W, H, 1.2 * W, 1.2 * W, background_color=torch.tensor(BG))
    rs = make_raster_settings(pc, torch.tensor(c2w, dtype=torch.float32), 3, device='cpu')
    np.testing.assert_allclose(rs.viewmatrix.numpy(), view.detach().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(rs.projmatrix.numpy(), proj.detach().numpy(), rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, name, **values):
    args = []
    for t, arg in protos[name][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, name)(*args)


def test_e_entry_points_are_exported_and_declared(lib):
    protos = _lib.parse_header()
    for name in SYMBOLS:
        assert name in protos and hasattr(lib, name), name
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 14
    aux = [a for _, a in protos['nrc_gs_backward_aux_band'][1]]
    mine = [a for _, a in protos['nrc_gs_backward_pose_band'][1]]
    assert mine == aux[:-1] + ['pose_partials', 'dL_dcamera', 'stream']            # every argument of the aux entry point, the two new ones, the stream
    assert [a for _, a in protos['nrc_gs_camera_block_backward'][1]] == ['c2w_dev', 'proj_t_dev', 'dL_dcamera', 'dL_dc2w_out', 'stream']
    assert not any('rest_step' in n and 'pose' in n for n in protos)                # no camera gradient in the in-backward Adam step


def test_e_workspace_size(lib):
    assert lib.nrc_gs_pose_partials_floats(-1) == NRC_ERR_INVALID
    assert lib.nrc_gs_pose_partials_floats(0) == 32                                 # P == 0 is accepted: one slab, never read
    assert lib.nrc_gs_pose_partials_floats(1) == lib.nrc_gs_pose_partials_floats(128) == 32
    assert lib.nrc_gs_pose_partials_floats(129) == 64
    big = lib.nrc_gs_pose_partials_floats(2 ** 31 - 1)
    assert big % 32 == 0 and big == lib.nrc_gs_pose_partials_floats(10 ** 7)         # the number of workgroups is capped


@pytest.mark.parametrize('begin,n', [(-1, 2), (0, 0), (3, 2), (4, 1), (0, 5), (2, -1)])
def test_e_a_bad_band_is_invalid_before_any_device_call(lib, begin, n):
    protos = _lib.parse_header()
    assert _call(lib, protos, 'nrc_gs_backward_pose_band') == NRC_ERR_INVALID        # H = 0: no band is valid
    assert _call(lib, protos, 'nrc_gs_backward_pose_band', P=0, W=64, H=64, tile_row_begin=begin, n_tile_rows=n) == NRC_ERR_INVALID


def test_e_workspace_checks_run_before_any_device_call(lib):
    """Host memory stands in for the device buffers: a refused call touches none of them, and no HIP call is made in front of the checks."""
    protos = _lib.parse_header()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    host = (ctypes.c_float * 38)(*([0.0] * 38))
    common = dict(P=0, W=64, H=64, tile_row_begin=0, n_tile_rows=4, tan_fovx=0.5, tan_fovy=0.5, camera_dev=ctypes.cast(host, ctypes.c_void_p))
    dcam = ctypes.c_void_p(base + 128)
    assert _call(lib, protos, 'nrc_gs_backward_pose_band', dL_dcamera=dcam, **common) == NRC_ERR_INVALID                                       # no workspace
    assert _call(lib, protos, 'nrc_gs_backward_pose_band', dL_dcamera=dcam, pose_partials=ctypes.c_void_p(base + 4), **common) == NRC_ERR_INVALID   # misaligned
    # P == 0 without a camera gradient is nrc_gs_backward_aux_band itself: accepted, nothing to launch
    assert _call(lib, protos, 'nrc_gs_backward_pose_band', **common) == NRC_OK
    assert _call(lib, protos, 'nrc_gs_backward_pose_band', pose_partials=ctypes.c_void_p(base + 4), **common) == NRC_OK                   # (ignored without dL_dcamera)
    for missing in ('c2w_dev', 'proj_t_dev', 'dL_dcamera', 'dL_dc2w_out'):
        ptrs = {k: ctypes.c_void_p(base) for k in ('c2w_dev', 'proj_t_dev', 'dL_dcamera', 'dL_dc2w_out') if k != missing}
        assert _call(lib, protos, 'nrc_gs_camera_block_backward', **ptrs) == NRC_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- pose recovery on the reference alone
def pose_from(c2w_true, dt, rotvec):
    """c2w = [exp([rotvec]_x) R_true | t_true + dt] with torch ops (differentiable)."""
    z = rotvec.new_zeros(())
    skew = torch.stack([torch.stack([z, -rotvec[2], rotvec[1]]), torch.stack([rotvec[2], z, -rotvec[0]]), torch.stack([-rotvec[1], rotvec[0], z])])
    rot = torch.linalg.matrix_exp(skew) @ c2w_true[:3, :3]
    return torch.cat([rot, (c2w_true[:3, 3] + dt)[:, None]], dim=1)


START_DT = 0.05 * np.array([0.6, -0.48, 0.64])
START_ROT = np.array([0.01, -0.02, 0.015])


def test_f_adam_recovers_the_pose_on_the_reference():
    """Scene A frozen, the target rendered at the true pose; the start is off by 0.05 (0.6, -0.48, 0.64) in translation and by the rotation vector (0.01, -0.02, 0.015)
    (c2w = [exp([w]x) R | t + dt]); Adam, lr 2e-3, 100 steps on dt and w in float64, the loss the mean squared pixel difference, the gradient the reference's.
    Both errors must end below half their start.  Measured: translation 0.0500 -> 0.0149, rotation 0.0269 -> 0.0051, loss 7.30e-3 -> 2.02e-5."""
    sc, cam = _scene_a()
    c2w_true = torch.tensor(scenes.orbit_pose(*POSE), dtype=torch.float64)
    proj_t = torch.tensor(_proj_t(cam))

    def camera(pose):
        rot, pos = pose[:3, :3], pose[:3, 3]
        last_row = torch.cat([-(rot.T @ pos), pose.new_ones(1)])
        view = torch.cat([torch.cat([rot, pose.new_zeros(3, 1)], dim=1), last_row[None]], dim=0)
        return view, view @ proj_t, pos

    def cam_dict(view, proj, pos):
        return dict(cam, viewmatrix=view.detach().numpy().copy(), projmatrix=proj.detach().numpy().copy(), campos=pos.detach().numpy().copy())

    with torch.no_grad():
        target = _forward(sc, cam_dict(*camera(c2w_true)))[0]
    dt = torch.tensor(START_DT, requires_grad=True)
    rv = torch.tensor(START_ROT, requires_grad=True)
    opt = torch.optim.Adam([dt, rv], lr=2e-3)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        view, proj, pos = camera(pose_from(c2w_true, dt, rv))
        c = cam_dict(view, proj, pos)
        image, _, st = _forward(sc, c)
        diff = image - target
        losses.append(float((diff * diff).mean()))
        want = expected_camera_gradients(sc, c, st, oracle.gs_backward(st, 2.0 * diff / diff.size))
        ((view * torch.tensor(want['view'][0])).sum() + (proj * torch.tensor(want['proj'][0])).sum() + (pos * torch.tensor(want['campos'][0])).sum()).backward()
        opt.step()
    e_t, e_r = float(dt.detach().norm()), float(rv.detach().norm())
    print(f'translation error {np.linalg.norm(START_DT):.4f} -> {e_t:.4f}   rotation error {np.linalg.norm(START_ROT):.4f} -> {e_r:.4f}   '
          f'loss {losses[0]:.2e} -> {losses[-1]:.2e}')
    assert e_t < 0.5 * np.linalg.norm(START_DT) and e_r < 0.5 * np.linalg.norm(START_ROT)
