"""The float64 reference of the rasterizer's camera gradients (camera_grad=True), built from the CPU oracle as it stands (nothing under oracle/ changes).

The oracle's backward pass returns per-Gaussian gradients (mean2D, conic, mean3D) but none for the camera.  Every camera gradient is a sum over the Gaussians
of a forward quantity times such a per-Gaussian gradient, so this module restates the chain of the per-Gaussian backward in numpy float64 -- conic -> the
two rows Mx, My of J W -> the projection Jacobian's entries -> the view-space mean t -> the view matrix; mean2D -> the homogeneous mean -> the projection
matrix; and the SH direction -> the camera position -- and adds the addends up.  With V[k][j] = viewmatrix[k, j], Pm[k][c] = projmatrix[k, c], m the mean:

    dV[k][0] = sum J00 dMx[k] + m_k dtx          dV[k][1] = sum J11 dMy[k] + m_k dty          dV[k][2] = sum J02 dMx[k] + J12 dMy[k] + m_k (dtz + gz)
    dV[3][:] = sum (dtx, dty, dtz + gz)          dPm[k][c] = sum m_k dmh_c,  dPm[3][c] = sum dmh_c,  dmh = (mw g2x, mw g2y, 0, -(mul1 g2x + mul2 g2y))
    dcampos  = -sum (the oracle's dL/dmean3D - its part through the view matrix - its part through the projection matrix)      (what is left is the SH part)

gz is dL/dz of the depth map (gs_depth_alpha_ref: the colour gradient of plane 0 of the second oracle run); V[.][3] and Pm[.][2] are not read by the
rasterizer: exactly zero.  Each gradient comes with `mag`, the sum of the absolute values of its per-Gaussian addends: the scale its error is judged by.
tests/test_gs_pose_grad_ref_cpu.py holds all of this against central differences of oracle.gs_forward(dtype=float64)."""
import numpy as np

import oracle
from tests.gs_depth_alpha_ref import expected_gradients


def fov_clamped(sc, cam, st):
    """Visible Gaussians whose view-space x / z or y / z lies outside the 1.3 tan(fov / 2) clamp of the projection Jacobian (a kink of the forward)."""
    vm = np.asarray(cam['viewmatrix'], np.float64)
    t = np.asarray(sc['means3D'], np.float64) @ vm[:3, :3] + vm[3, :3]
    vis = np.asarray(st.radii) > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        out = (np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam['tanfovx']) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam['tanfovy'])
    return vis & out


def expected_camera_gradients(sc, cam, st, oracle_grads, gz=None):
    """dict(view=(grad (4,4), mag (4,4)), proj=(grad (4,4), mag (4,4)), campos=(grad (3,), mag (3,))) in float64.
    sc: the scene (means3D); cam: tests.scenes.gs_camera's dict; st: the oracle's forward state (radii, cov3D, inputs); oracle_grads: oracle.gs_backward's
    dict (mean2D, conic, mean3D are read -- with depth / alpha gradients, gs_depth_alpha_ref.expected_gradients' sums); gz (P,): dL/dz per Gaussian or None."""
    f = np.float64
    vm, pm = np.asarray(cam['viewmatrix'], f), np.asarray(cam['projmatrix'], f)
    vis = np.asarray(st.radii) > 0
    m = np.asarray(sc['means3D'], f)[vis]
    n = m.shape[0]
    cov = np.asarray(st.cov3D, f)[vis]
    g2 = np.asarray(oracle_grads['mean2D'], f)[vis]
    gc = np.asarray(oracle_grads['conic'], f)[vis]
    gmean = np.asarray(oracle_grads['mean3D'], f)[vis]
    gzv = np.zeros(n, f) if gz is None else np.asarray(gz, f)[vis]
    W, H = cam['width'], cam['height']
    tanx, tany = f(cam['tanfovx']), f(cam['tanfovy'])
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    # forward quantities
    t = m @ vm[:3, :3] + vm[3, :3]
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    tcx, tcy, tcz = np.clip(txtz, -limx, limx) * t[:, 2], np.clip(tytz, -limy, limy) * t[:, 2], t[:, 2]
    gmx, gmy = (np.abs(txtz) <= limx).astype(f), (np.abs(tytz) <= limy).astype(f)
    j00, j02 = fx / tcz, -(fx * tcx) / (tcz * tcz)
    j11, j12 = fy / tcz, -(fy * tcy) / (tcz * tcz)
    Mx = j00[:, None] * vm[None, :3, 0] + j02[:, None] * vm[None, :3, 2]
    My = j11[:, None] * vm[None, :3, 1] + j12[:, None] * vm[None, :3, 2]
    S = np.empty((n, 3, 3), f)
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2] = (cov[:, k] for k in range(6))
    S[:, 1, 0], S[:, 2, 0], S[:, 2, 1] = S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
    sx, sy = np.einsum('nij,nj->ni', S, Mx), np.einsum('nij,nj->ni', S, My)
    a = (Mx * sx).sum(1) + 0.3
    b = (Mx * sy).sum(1)
    c = (My * sy).sum(1) + 0.3
    # conic -> cov2D -> Mx, My (the statements of the per-Gaussian backward)
    gcx, gcy, gcz = gc[:, 0], gc[:, 1], gc[:, 3]
    denom = a * c - b * b
    d2 = 1.0 / (denom * denom + 0.0000001)
    dL_da = d2 * (-c * c * gcx + 2 * b * c * gcy + (denom - a * c) * gcz)
    dL_dc = d2 * (-a * a * gcz + 2 * a * b * gcy + (denom - a * c) * gcx)
    dL_db = d2 * 2 * (b * c * gcx - (denom + 2 * b * b) * gcy + a * b * gcz)
    dMx = 2 * sx * dL_da[:, None] + sy * dL_db[:, None]
    dMy = 2 * sy * dL_dc[:, None] + sx * dL_db[:, None]
    dJ00, dJ02 = dMx @ vm[:3, 0], dMx @ vm[:3, 2]
    dJ11, dJ12 = dMy @ vm[:3, 1], dMy @ vm[:3, 2]
    tz = 1.0 / tcz
    tz2, tz3 = tz * tz, tz * tz * tz
    dtx = gmx * -fx * tz2 * dJ02
    dty = gmy * -fy * tz2 * dJ12
    dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2 * fx * tcx) * tz3 * dJ02 + (2 * fy * tcy) * tz3 * dJ12
    dt = np.stack([dtx, dty, dtz + gzv], 1)
    # mean2D -> homogeneous mean
    mh = m @ pm[:3, :] + pm[3, :]
    mw = 1.0 / (mh[:, 3] + 0.0000001)
    mul1, mul2 = mh[:, 0] * mw * mw, mh[:, 1] * mw * mw
    dmh = np.stack([mw * g2[:, 0], mw * g2[:, 1], np.zeros(n, f), -(mul1 * g2[:, 0] + mul2 * g2[:, 1])], 1)
    # per-Gaussian addends (n, 4, 4) / (n, 3)
    aV = np.zeros((n, 4, 4), f)
    aV[:, :3, 0] = j00[:, None] * dMx
    aV[:, :3, 1] = j11[:, None] * dMy
    aV[:, :3, 2] = j02[:, None] * dMx + j12[:, None] * dMy
    mV = np.abs(aV)
    mt = np.zeros((n, 4, 4), f)
    mt[:, :3, :3] = m[:, :, None] * dt[:, None, :]
    mt[:, 3, :3] = dt
    aV, mV = aV + mt, mV + np.abs(mt)
    aP = np.zeros((n, 4, 4), f)
    aP[:, :3, :] = m[:, :, None] * dmh[:, None, :]
    aP[:, 3, :] = dmh
    view_part = dt @ vm[:3, :3].T                       # dL/dmean through t = m V + V[3]
    proj_part = dmh @ pm[:3, :].T                       # ... through mh = m Pm + Pm[3]
    if st.inputs['shs'] is None or st.D == 0:           # precomputed colours or a constant colour: no view direction, structurally zero
        aC = np.zeros((n, 3), f)
    else:
        aC = -(gmean - view_part - proj_part)
        # a Gaussian whose colour received no gradient (every channel clamped, or no colour loss at all) has no SH part: the subtraction would leave the
        # rounding of a float32 oracle there
        aC[~np.asarray(oracle_grads['color'], f)[vis].any(1)] = 0.0
    return dict(view=(aV.sum(0), mV.sum(0)), proj=(aP.sum(0), np.abs(aP).sum(0)), campos=(aC.sum(0), np.abs(aC).sum(0)))


def oracle_gradients_with_maps(st, st2, cam, g_rgb, g_d, g_a):
    """(grads, gz) for expected_camera_gradients when the depth and alpha maps take part: gs_depth_alpha_ref.expected_gradients' sums of the two oracle
    backward passes, the conic gradient summed the same way, and gz = dL/dz per Gaussian (the colour gradient of plane 0 of the second run)."""
    grads = expected_gradients(st, st2, cam, g_rgb, g_d, g_a)
    second = oracle.gs_backward(st2, np.stack([g_d, g_a, np.zeros_like(g_d)]))
    grads['conic'] = oracle.gs_backward(st, g_rgb)['conic'] + second['conic']
    return grads, second['color'][:, 0]


def c2w_gradient(c2w, proj_t, dview, dproj, dcampos):
    """dL/dc2w (3, 4) of the camera that make_raster_settings builds from a pose: viewmatrix = [[R, 0], [-(R^T t)^T, 1]], projmatrix = viewmatrix @ proj_t,
    campos = t (c2w = [R | t])."""
    f = np.float64
    c2w, proj_t, dview, dproj, dcampos = (np.asarray(v, f) for v in (c2w, proj_t, dview, dproj, dcampos))
    dV = dview + dproj @ proj_t.T
    R, t = c2w[:3, :3], c2w[:3, 3]
    out = np.zeros((3, 4), f)
    out[:, :3] = dV[:3, :3] - t[:, None] * dV[3, None, :3]
    out[:, 3] = dcampos - R @ dV[3, :3]
    return out


def c2w_gradient_mag(c2w, proj_t, dview, dproj, dcampos):
    """The sum of the absolute values of the addends of c2w_gradient, entry by entry (3, 4)."""
    f = np.float64
    c2w, proj_t, dview, dproj, dcampos = (np.abs(np.asarray(v, f)) for v in (c2w, proj_t, dview, dproj, dcampos))
    dV = dview + dproj @ proj_t.T
    R, t = c2w[:3, :3], c2w[:3, 3]
    out = np.zeros((3, 4), f)
    out[:, :3] = dV[:3, :3] + t[:, None] * dV[3, None, :3]
    out[:, 3] = dcampos + R @ dV[3, :3]
    return out
