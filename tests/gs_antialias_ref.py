"""Float64 references and error budgets for the anti-aliased splats of the 3DGS rasterizer (nerficg_amd/csrc/gs_raster.hip: preprocess_one<true>,
preprocess_bw_one<true>; C ABI group 27) and for the 3-D smoothing filter (csrc/gs_densify.hip: k_filter3d).  Plain module: no test functions.  Used by
tests/test_gs_antialias_ref_cpu.py and tests/test_gpu_gs_antialias.py.

The compensation (comp64)
-------------------------
With Mx, My the two rows of J W (restated as tests/gs_pose_grad_ref.py restates them) and Sigma the saved cov3D, all float32 values promoted:
    a0 = Mx Sigma Mx   b = Mx Sigma My   c0 = My Sigma My      a = a0 + 0.3f   c = c0 + 0.3f      det0 = a0 c0 - b^2   det1 = a c - b^2
    rho = det0 / det1          comp = sqrt(max(0.000025f, rho))                                    (0.3f and 0.000025f: the float32 constants promoted)
The blended opacity is o comp.  Its backward, with g = dL/d(o comp): dL/do = g comp, and for rho above the floor, k = g o / (2 comp),
    dL/da0 += k (c0 det1 - c det0) / det1^2      dL/dc0 += k (a0 det1 - a det0) / det1^2      dL/db += k (-2 b) (det1 - det0) / det1^2

The budget of comp (u = 2^-24, gamma(C) = C u / (1 - C u) as in gs_grad_ref.py)
------------------
    budget(rho) = gamma(C_RHO) (|a0 c0| + b^2) / det1          budget(comp) = budget(rho) / (2 comp) + gamma(2) comp      (at the floor: gamma(1) comp)
C_RHO = 160 counts the roundings of the kernel's statements from its inputs to rho, relative to the products the last statements see:
    t = W m + t0 (xform43: 6), the Jacobian's entries fx / tz, -(fx tx) / tz^2 (3), Mx = J W (two products, one sum: 3 on top) -- 12 per element of Mx;
    sx = Sigma Mx (three products, two sums: 5), a0 = Mx . sx (5), Mx entering twice: 2 x 12 + 5 + 5 = 34, with the 1-ulp differences of focal_x and of the
    limits of the Jacobian's clamp rounded up to 38 for each of a0, b, c0;
    det0 = a0 c0 - b^2: the two products carry 2 x 38, plus a product and the difference: 78, relative to |a0 c0| + b^2;
    det1 = a c - b^2 likewise with one more rounding per dilated term: 80, relative to a c + b^2; it enters rho as rho (delta det1) / det1, and
    rho (a c + b^2) <= |a0 c0| + b^2 (cross-multiplied: a0 c0 b^2 <= a c b^2), so it is carried by the same magnitude expression;
    the division: 1.  78 + 80 + 1 = 159, rounded to 160.
sqrt and the product with max() add gamma(2) comp.  In raw-parameter mode o = 1 / (1 + expf(-x)) adds gamma(C_SIGMOID) o, C_SIGMOID = 5 (expf 2 ulp, the sum,
the division, one of margin for the negation's exact result being used by a 1-ulp exp).  `classify` holds every Gaussian's rho against the floor with a margin
of ten budgets: the tests admit no scene in which one is closer.

The extra gradient as an equivalent conic gradient (equivalent_conic), and the leaves (aa_leaf_ref)
------------------------------------------------------------------------------------------------
preprocess_bw_one chains (dL_da, dL_dc, dL_db) to cov3D, scales, rotations and means; the float64 oracle restates that chain from a CONIC gradient:
    dL_da = d (-c^2 gx + 2 b c gy + (denom - a c) gz)    dL_dc = d (-a^2 gz + 2 a b gy + (denom - a c) gx)    dL_db = 2 d (b c gx - (denom + 2 b^2) gy + a b gz)
with denom = a c - b^2 and d = 1 / (denom^2 + 1e-7).  These three lines are a 3 x 3 linear system per Gaussian: solving it for the three extra terms gives the
conic gradient g_equiv that the unchanged oracle turns into exactly the extra leaf gradients.  The anti-aliased leaves are therefore gs_grad_ref.LeafRef on
    S'_opacity = S_opacity comp          S'_conic = S_conic + g_equiv
with S the blend sums (of the kernel's own state: the blend sees o comp and nothing else of the flag).  Magnitudes and budgets travel the same way:
    A'_opacity = A_opacity comp                      B'_opacity = B_opacity comp + |S_opacity| budget(comp) + gamma(1) |S'_opacity|
    A'_conic   = A_conic + |M^-1| A_extra            B'_conic   = B_conic + |M^-1| B_extra
A_extra: the three terms with g replaced by A_opacity and every difference by the sum of the absolute values of its two products.
B_extra(a0) = (B_opacity o / (2 comp)) E_a + |S_opacity| o / (2 comp) [ (budget(comp) / comp + gamma(3)) E_a + (|c0| ddet1 + |c| ddet0) / det1^2
              + gamma(C_ABC + 3) E_a + (|N_a| / det1^2) (2 ddet1 / det1 + gamma(4)) ]
with N_a = c0 det1 - c det0, E_a = (|c0 det1| + |c det0|) / det1^2, ddet0 = gamma(80) (|a0 c0| + b^2), ddet1 = gamma(80) (a c + b^2), C_ABC = 38 (the error
of c0 and c themselves); c0 and b likewise (for b: N_b = -2 b (det1 - det0), the difference's error ddet1 + ddet0).  The part of B_extra that is relative
(everything but the fixed and tiny parts inside B_opacity) is asserted <= GATE A_extra, the project's 2e-3.
At or below the floor there is no extra term, S'_conic = S_conic, and comp is the constant sqrt(0.000025f).

The 3-D filter (filter3d_ref)
-----------------------------
The loop of Mip-Splatting's compute_3D_filter in float64 on the promoted float32 inputs, with the per-view ratio z / fx: see its docstring."""
from __future__ import annotations

import math

import numpy as np

from tests import gs_grad_ref as R

f64 = np.float64
DILATION = float(np.float32(0.3))
FLOOR = float(np.float32(0.000025))
C_RHO, C_DET, C_ABC, C_SIGMOID = 160, 80, 38, 5
gamma = R.gamma


# ------------------------------------------------------------------------------------------------------------------------ comp
def cov2d(means3D, cov3D, cam):
    """(a0, b, c0), each (P,) float64: the projected covariance before the dilation, from float32 values promoted.  cam: tests.scenes.gs_camera's dict.
    Rows of Gaussians behind the camera hold whatever the arithmetic gives (nan / inf allowed): callers select the visible ones."""
    vm = np.asarray(cam['viewmatrix'], f64)
    m = np.asarray(means3D, f64)
    cov = np.asarray(cov3D, f64)
    W, H = cam['width'], cam['height']
    tanx, tany = float(np.float32(cam['tanfovx'])), float(np.float32(cam['tanfovy']))
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    with np.errstate(all='ignore'):
        t = m @ vm[:3, :3] + vm[3, :3]
        limx, limy = 1.3 * tanx, 1.3 * tany
        tcx, tcy, tcz = np.clip(t[:, 0] / t[:, 2], -limx, limx) * t[:, 2], np.clip(t[:, 1] / t[:, 2], -limy, limy) * t[:, 2], t[:, 2]
        j00, j02 = fx / tcz, -(fx * tcx) / (tcz * tcz)
        j11, j12 = fy / tcz, -(fy * tcy) / (tcz * tcz)
        Mx = j00[:, None] * vm[None, :3, 0] + j02[:, None] * vm[None, :3, 2]
        My = j11[:, None] * vm[None, :3, 1] + j12[:, None] * vm[None, :3, 2]
        S = np.empty((m.shape[0], 3, 3), f64)
        S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2] = (cov[:, k] for k in range(6))
        S[:, 1, 0], S[:, 2, 0], S[:, 2, 1] = S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
        sx, sy = np.einsum('nij,nj->ni', S, Mx), np.einsum('nij,nj->ni', S, My)
        return (Mx * sx).sum(1), (Mx * sy).sum(1), (My * sy).sum(1)


class Comp:
    """comp64 and everything the tests need of it, per Gaussian (P,): a0, b, c0, a, c, det0, det1, rho, comp, floor (rho <= FLOOR), b_rho, b_comp."""

    def __init__(self, a0, b, c0):
        self.a0, self.b, self.c0 = (np.asarray(v, f64) for v in (a0, b, c0))
        with np.errstate(all='ignore'):
            self.a, self.c = self.a0 + DILATION, self.c0 + DILATION
            self.det0 = self.a0 * self.c0 - self.b * self.b
            self.det1 = self.a * self.c - self.b * self.b
            self.rho = self.det0 / self.det1
            self.floor = ~(self.rho > FLOOR)
            self.comp = np.sqrt(np.maximum(FLOOR, np.nan_to_num(self.rho, nan=0.0)))
            self.m0 = np.abs(self.a0 * self.c0) + self.b * self.b
            self.m1 = np.abs(self.a * self.c) + self.b * self.b
            self.b_rho = gamma(C_RHO) * self.m0 / self.det1
            self.b_comp = np.where(self.floor, gamma(1) * self.comp, self.b_rho / (2.0 * self.comp) + gamma(2) * self.comp)


def comp64(means3D, cov3D, cam):
    return Comp(*cov2d(means3D, cov3D, cam))


def classify(q, visible):
    """Asserts that every visible Gaussian's rho is at least ten budgets away from the floor; returns the floor mask of the visible ones."""
    vis = np.asarray(visible, bool)
    margin = np.abs(q.rho[vis] - FLOOR)
    need = 10.0 * q.b_rho[vis]
    assert np.isfinite(q.rho[vis]).all()
    assert (margin >= need).all(), f'{int((margin < need).sum())} Gaussians lie within ten budgets of the floor: worst margin / budget {(margin / q.b_rho[vis]).min():.3g}'
    return q.floor & vis


def sigmoid64(logit):
    return 1.0 / (1.0 + np.exp(-np.asarray(logit, f64)))


# ------------------------------------------------------------------------------------------------------------------------ the extra gradient
def extra_abc(q, g, o):
    """The three added terms (da0, dc0, db), each (P,) float64, for g = dL/d(o comp) and the opacities o; zero at or below the floor."""
    g, o = np.asarray(g, f64), np.asarray(o, f64)
    with np.errstate(all='ignore'):
        k = g * o / (2.0 * q.comp)
        d2 = q.det1 * q.det1
        da = k * (q.c0 * q.det1 - q.c * q.det0) / d2
        dc = k * (q.a0 * q.det1 - q.a * q.det0) / d2
        db = k * (-2.0 * q.b) * (q.det1 - q.det0) / d2
    z = lambda v: np.where(q.floor, 0.0, np.nan_to_num(v))
    return z(da), z(dc), z(db)


def extra_abc_budget(q, S_op, A_op, B_op, Brel_op, o):
    """(A_extra, B_extra, Brel_extra), each (P, 3) in the order (a0, c0, b): magnitudes and budgets of extra_abc's terms for g = the blend's opacity sum with
    magnitude A_op, budget B_op and relative part Brel_op (docstring)."""
    o = np.abs(np.asarray(o, f64))
    with np.errstate(all='ignore'):
        h = o / (2.0 * q.comp)
        d2 = q.det1 * q.det1
        dd0, dd1 = gamma(C_DET) * q.m0, gamma(C_DET) * q.m1
        N = [q.c0 * q.det1 - q.c * q.det0, q.a0 * q.det1 - q.a * q.det0, -2.0 * q.b * (q.det1 - q.det0)]
        E = [(np.abs(q.c0 * q.det1) + np.abs(q.c * q.det0)) / d2, (np.abs(q.a0 * q.det1) + np.abs(q.a * q.det0)) / d2,
             2.0 * np.abs(q.b) * (np.abs(q.det1) + np.abs(q.det0)) / d2]
        D = [(np.abs(q.c0) * dd1 + np.abs(q.c) * dd0) / d2, (np.abs(q.a0) * dd1 + np.abs(q.a) * dd0) / d2, 2.0 * np.abs(q.b) * (dd1 + dd0) / d2]
        A, B, Brel = [], [], []
        for n, e, d in zip(N, E, D):
            own = (q.b_comp / q.comp + gamma(3)) * e + d + gamma(C_ABC + 3) * e + (np.abs(n) / d2) * (2.0 * dd1 / np.abs(q.det1) + gamma(4))
            A.append(A_op * h * e)
            B.append(B_op * h * e + np.abs(S_op) * h * own)
            Brel.append(Brel_op * h * e + np.abs(S_op) * h * own)
    z = lambda v: np.where(q.floor[:, None], 0.0, np.nan_to_num(np.stack(v, 1)))
    return z(A), z(B), z(Brel)


def conic_system(q):
    """(P, 3, 3): the matrix of the three lines of preprocess_bw_one that turn a conic gradient (gx, gy, gz) into (dL_da, dL_dc, dL_db), the +1e-7 included."""
    a, b, c = q.a, q.b, q.c
    with np.errstate(all='ignore'):
        denom = a * c - b * b
        d = 1.0 / (denom * denom + 0.0000001)
        M = np.stack([np.stack([-c * c, 2 * b * c, denom - a * c], -1), np.stack([denom - a * c, 2 * a * b, -a * a], -1),
                      2.0 * np.stack([b * c, -(denom + 2 * b * b), a * b], -1)], 1) * d[:, None, None]
    return M


def equivalent_conic(q, extra, live):
    """g_equiv (P, 3) = (xx, xy, yy) with conic_system(q) g_equiv = extra (P, 3 in the order a0, c0, b) for the rows of `live`; zero elsewhere.  Also returns
    |M^-1| (P, 3, 3) for the magnitudes."""
    P = q.a.shape[0]
    M = conic_system(q)
    g, Minv_abs = np.zeros((P, 3)), np.zeros((P, 3, 3))
    idx = np.nonzero(np.asarray(live, bool))[0]
    if idx.size:
        Minv = np.linalg.inv(M[idx])
        g[idx] = np.einsum('nij,nj->ni', Minv, np.asarray(extra, f64)[idx])
        Minv_abs[idx] = np.abs(Minv)
    return g, Minv_abs


def blend_relative_part(ref):
    """The relative part of gs_grad_ref.blend_budget (order='kernel') per sum, (P, NQ): B minus the fixed and tiny parts."""
    return ref['R'] + gamma(ref['tiles'] + 2)[:, None] * ref['A']


def aa_sums(q, ref, B, o, visible):
    """(ref', B'): the transformed sums, magnitudes and budgets of the docstring.  ref: BlendRef.sums' dict of the kernel's state (whose opacity is o comp);
    B: blend_budget's (P, NQ); o (P,): the opacities in front of the compensation; visible (P,) bool."""
    vis = np.asarray(visible, bool)
    S, A = ref['S'].copy(), ref['A'].copy()
    B = B.copy()
    comp = np.where(vis, q.comp, 0.0)
    b_comp = np.where(vis, q.b_comp, 0.0)
    S_op, A_op, B_op = ref['S'][:, 3], ref['A'][:, 3], B[:, 3].copy()
    live = vis & ~q.floor
    extra = np.stack(extra_abc(q, S_op, o), 1) * live[:, None]
    A_x, B_x, Brel_x = extra_abc_budget(q, S_op, A_op, B_op, blend_relative_part(ref)[:, 3], o)
    A_x, B_x, Brel_x = (v * live[:, None] for v in (A_x, B_x, Brel_x))
    assert (Brel_x <= R.GATE * A_x).all(), 'the relative part of the extra terms\' budget exceeds the 2e-3 gate'
    g_eq, Minv_abs = equivalent_conic(q, extra, live)
    S[:, 3], A[:, 3] = S_op * comp, A_op * comp
    B[:, 3] = B_op * comp + np.abs(S_op) * b_comp + gamma(1) * np.abs(S[:, 3])
    S[:, 6:9] += g_eq
    A[:, 6:9] += np.einsum('nij,nj->ni', Minv_abs, A_x)
    B[:, 6:9] += np.einsum('nij,nj->ni', Minv_abs, B_x)
    out = dict(ref)
    out['S'], out['A'] = S, A
    return out, B


def aa_leaf_ref(c, r, q, o, visible):
    """gs_grad_ref.LeafRef of an anti-aliased call.  c: the case (tests/gs_grad_cases.py); r: gs_grad_cases.reference(...) built on the kernel's state of the
    anti-aliased run; q: comp64 of that state; o (P,) float64: the opacities in front of the compensation (raw form: sigmoid64 of the logits)."""
    ref2, B2 = aa_sums(q, r.ref, r.B, o, visible)
    leaf = R.LeafRef(r.st64, ref2, B2, view_z=np.asarray(c.cam['viewmatrix'])[:3, 2])
    if c.form == 'raw':
        leaf.to_raw_parameters(o, c.sc['scales'], c.sc['rotations'], np.sqrt((np.asarray(c.sc['raw']['quat'], f64) ** 2).sum(1)))
    return leaf


# ------------------------------------------------------------------------------------------------------------------------ the 3-D filter
SQRT_0_2 = 0.44721359549995793


def view_block(w2c, fx, fy, W, H):
    """One row of the (V, 20) float32 block nrc_gs_filter3d reads: the world-to-camera matrix row-major, fx, fy, W, H."""
    return np.concatenate([np.asarray(w2c, f64).reshape(16), [fx, fy, W, H]]).astype(np.float32)


def filter3d_ref(means3D, views):
    """(filter_3D (P,) float64, seen (P,) bool).  The loop of Mip-Splatting's compute_3D_filter over the rows of `views` ((V, 20) float32, view_block) in float64
    on the promoted values, in the kernel's order of operations: z first; a view sees a Gaussian iff z > 0.2 and x / z fx + W / 2, y / z fy + H / 2 lie in
    [-0.15 W, 1.15 W] x [-0.15 H, 1.15 H]; filter = sqrt(0.2) min over the seeing views of z / fx (the published code: min z over the views divided by the
    largest fx -- equal for equal focal lengths).  A Gaussian no view sees gets the largest filter among the seen ones rounded to float32 (the kernel hands on
    the float32 value), 0 when none is seen."""
    p = np.asarray(means3D, np.float32).astype(f64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    dmin = np.full(p.shape[0], np.inf)
    seen = np.zeros(p.shape[0], bool)
    for row in np.asarray(views, np.float32).astype(f64):
        c = row
        zc = c[8] * x + c[9] * y + c[10] * z + c[11]
        xc = c[0] * x + c[1] * y + c[2] * z + c[3]
        yc = c[4] * x + c[5] * y + c[6] * z + c[7]
        fx, fy, W, H = c[16], c[17], c[18], c[19]
        with np.errstate(all='ignore'):
            px, py = xc / zc * fx + 0.5 * W, yc / zc * fy + 0.5 * H
            ok = (zc > 0.2) & (px >= -0.15 * W) & (px <= 1.15 * W) & (py >= -0.15 * H) & (py <= 1.15 * H)
            dmin = np.where(ok, np.minimum(dmin, zc / fx), dmin)
        seen |= ok
    out = np.where(seen, SQRT_0_2 * np.where(seen, dmin, 0.0), 0.0)
    if seen.any():
        out[~seen] = float(np.float32(out[seen]).max())
    return out, seen


# ------------------------------------------------------------------------------------------------------------------------ the cases
def _quat_of(Rm):
    """Unit quaternion (r, x, y, z) of a rotation matrix (trace branch only where it is safe, else the largest diagonal)."""
    Rm = np.asarray(Rm, f64)
    tr = np.trace(Rm)
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (Rm[2, 1] - Rm[1, 2]) / s, (Rm[0, 2] - Rm[2, 0]) / s, (Rm[1, 0] - Rm[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(Rm)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(Rm[i, i] - Rm[j, j] - Rm[k, k] + 1.0) * 2
        v = [0.0, 0.0, 0.0]
        v[i], v[j], v[k] = 0.25 * s, (Rm[j, i] + Rm[i, j]) / s, (Rm[k, i] + Rm[i, k]) / s
        q = [(Rm[k, j] - Rm[j, k]) / s] + v
    q = np.asarray(q, f64)
    return (q / np.linalg.norm(q)).astype(np.float32)


def needle_scene(n=129, seed=5):
    """The base generator's scene with every fourth Gaussian replaced by a splat that hits the floor of comp: alternately a point (three scales of 1e-4) and a
    needle along the camera's right axis (scales 0.3, 1e-5, 1e-5: a0 large, c0 and b tiny, so that |a0 c0| + b^2, the scale of rho's error, is tiny too).  They
    sit near the view axis with opacity 0.95: o comp = 0.00475 >= 1/255, the pixels next to their centres blend them."""
    from tests import gs_grad_cases as C
    from tests import scenes
    sc = scenes.gs_random_scene(n, seed=seed, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=3)
    c2w = scenes.orbit_pose(*C.POSE)
    q_right = _quat_of(c2w[:3, :3])
    rng = np.random.default_rng(seed + 1)
    for j, i in enumerate(range(0, n, 4)):
        local = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)])
        sc['means3D'][i] = (c2w[:3, :3] @ local).astype(np.float32)
        sc['opacities'][i] = 0.95
        if j % 2 == 0:
            sc['scales'][i] = 1e-4
        else:
            sc['scales'][i] = (0.3, 1e-5, 1e-5)
            sc['rotations'][i] = q_right
    return sc


def cases():
    """name -> zero-argument maker of a gs_grad_cases case.  P in {1, 127, 128, 129, 300} (the 128-Gaussian workgroup edge), 16 x 16 and 40 x 24 (partial tiles),
    SH degree 0 and 3, one (P, M, 3) SH tensor and dc + rest, scales + rotations and cov3D_precomp, colors_precomp, raw and activated parameters, and the
    needle scene."""
    from tests import gs_grad_cases as C
    from tests import scenes

    def scene(n, deg=3, seed=11):
        return scenes.gs_random_scene(n, seed=seed, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=deg)

    def one():
        sc = scene(1, 0)
        sc['means3D'][:] = (0.05, -0.03, 0.02)
        sc['opacities'][:] = 0.7
        return C._case('p1-16x16-deg0', sc, w=16, h=16)

    def precomp():
        sc = scene(129)
        sc['cov3D_precomp'] = C.forward(C._case('tmp', sc, w=16, h=16))[0].cov3D.copy()
        sc['colors_precomp'] = np.random.default_rng(1).random((129, 3)).astype(np.float32)
        return C._case('p129-16x16-precomp', sc, w=16, h=16, form='precomp')

    def raw():
        base = scene(128)
        rng = np.random.default_rng(7)
        rawp = dict(means3D=base['means3D'], dc=base['shs'][:, :1].copy(), rest=base['shs'][:, 1:].copy(),
                    logit=np.log(base['opacities'] / (1 - base['opacities'])).astype(np.float32)[:, None], log_scale=np.log(base['scales']).astype(np.float32),
                    quat=(base['rotations'] * rng.uniform(0.5, 2.0, size=(128, 1))).astype(np.float32))
        act, norm = C.activate(rawp)
        return C._case('p128-40x24-raw-split', C.with_activations(rawp, act, norm), w=40, h=24, form='raw')

    return {
        'p1-16x16-deg0': one,
        'p127-40x24-deg3': lambda: C._case('p127-40x24-deg3', scene(127), w=40, h=24),
        'p128-40x24-raw-split': raw,
        'p129-16x16-precomp': precomp,
        'p300-40x24-deg3-aux': lambda: C._case('p300-40x24-deg3-aux', scene(300), w=40, h=24, aux='all'),
        'needles-129-40x24': lambda: C._case('needles-129-40x24', needle_scene(), w=40, h=24),
    }
