"""Inputs, a float64 numpy restatement and a per-element error budget for the bilateral-grid kernels (nerficg_amd/csrc/bilateral_grid.hip, include/nerficg_hip.h
group 28, which states the definition).  Plain module: no test functions.  Used by tests/test_bilateral_grid_ref_cpu.py and tests/test_gpu_bilateral_grid.py.

The restatement
---------------
`evaluate` computes, in float64, the corrected image, the sliced matrices and the gradients w.r.t. the image and the grids; `tv` / `tv_grad` the
total-variation term and its gradient.  The luminance constants are the f32 numbers the kernel holds (f32(0.299), f32(0.587), f32(0.114)), so that the
comparison measures arithmetic, not constants.  Images are (H, W, 3) here; the tests permute for the (3, H, W) layout.

The inputs
----------
`draw`: colours in [0.02, 0.98], grids = identity + 0.2 N(0, 1), d_out N(0, 1) with a fifth of the elements exactly zero, all f32.  The derivative w.r.t. the
colour is discontinuous where a coordinate crosses a vertex, so the draw is repeated with the next seed (seed + 1000, + 2000, ...; only the offending pixels are
replaced, as in tests/map_losses_ref.py) until every pixel's c_z in float64 lies at least MARGIN = 1e-4 cell from an integer and g at least 1e-4 from 0 and 1;
c_x and c_y depend on the shapes alone and `margins` asserts the same distance for them (the case shapes are chosen so).  That is a condition on the inputs,
far above the f32 coordinate error (2u c <= 2e-6), and the reference alone satisfies it.  The kinks themselves are the named EXACT cases: dyadic grids,
colours and d_out, and colours for which the kernel's f32 luminance decides the same cell as float64 does -- black (g == 0), (2, 2, 2) and (-1, -1, -1)
(g outside [0, 1] by a clear margin: zero guidance gradient), power-of-two sizes whose pixel centres fall on vertices (W = 4 under Gw = 9, H = 2 under Gh = 5)
-- and white, where f32 gives g == 1 exactly ((f32(0.299) + f32(0.587)) + f32(0.114) rounds to 1) while the float64 sum of the same constants is
1 + 7.5e-9: for the exact cases `evaluate(..., g_f32=True)` takes g from the f32 sequence, which is the statement under test there (g == 1 takes the last
cell's slope), and everything behind it in float64.

The budget
----------
First-order propagation of u = 2^-24 through the kernel's own operation sequence (-ffp-contract=off: nothing is fused, every operation below rounds); every
f32 operation contributes u times its result on top of the propagated error of its operands (`e_` variables, absolute, float64, from the inputs alone).

  place     c_x = ((x + 0.5) / W) (Gw - 1)        e_c = 2u c                 (x + 0.5 is exact; one division, one product; the same along y)
            g = (CR p0 + CG p1) + CB p2           e_g = u (|t0| + |t1| + |t2|) + u |t0 + t1| + u |g|
            c_z = clamp(g) (L - 1)                e_c = (L - 1) e_g + u c_z
            f = c - i  (exact, i is exact by MARGIN)   e_f = e_c;   w1 = f: e_f,  w0 = 1 - f: e_f + u w0;   an axis of extent 1: f = 0, w = (1, 0), no error
  corner    wyx = wy wx                           e_wyx = e_wy wx + wy e_wx + u wyx
            w = wz wyx                            e_w = e_wz wyx + wz e_wyx + u w
  forward   A_c = sum of 8 products w G           e_A = sum (e_w |G| + u |w G|) + 7u sum |w G|            (7 additions; the sum of |addends| bounds every partial sum)
            out_r = ((A0 p0 + A1 p1) + A2 p2) + A3    e = sum_k e_A |q_k| + u sum_{k<3} |A_k p_k| + 3u sum_k |A_k q_k|,  q = (p0, p1, p2, 1)
  d_rgb     D_c = sum of 4 products wyx (G1 - G0) e_D = sum (e_wyx |dG| + u |dG| wyx + u |wyx dG|) + 3u sum |wyx dG|
            s_r = ((D0 p0 + D1 p1) + D2 p2) + D3  e_s = sum_k e_D |q_k| + u sum_{k<3} |D_k p_k| + 3u sum_k |D_k q_k|
            S = (d0 s0 + d1 s1) + d2 s2           e_S = sum_r |d_r| e_s + 3u sum_r |d_r s_r|              (one product, two additions)
            gz = S (L - 1)                        e_gz = (L - 1) e_S + u |gz|                             (exactly 0 outside 0 <= g <= 1)
            lin_k = (d0 A0k + d1 A1k) + d2 A2k    e_lin = sum_r |d_r| e_A + 3u sum_r |d_r A_rk|
            d_p_k = lin_k + coef_k gz             e = e_lin + |coef_k| e_gz + u |coef_k gz| + u |d_p_k|
  d_grids   m = d_r q_k (q_3 = 1: exact)          e_m = u |m|
            v = w m                               e_v = e_w |m| + w e_m + u |v|
            a wave sums 64 lanes with a butterfly (6 additions deep), the workgroup adds its four waves as (a + b) + (c + d) (2 deep): 8 additions,
            e = sum e_v + 8u sum |v|; the partial windows are summed in double (2^-53: dropped) and rounded once: + u |result|.  The direct path sums the
            same products in double: it stays inside.
  TV        d = G[i+1] - G[i]: u |d|, its square and every sum are double: e_TV = 2u TV + u TV (the result rounded once)
  TV grad   per axis d1 = G[i] - G[i-1], d2 = G[i+1] - G[i], s = d1 - d2: e_s = u (|d1| + |d2| + |s|);  gk = g k (k = f32(2 / (N count)): u; product: u);
            t = gk s: e_t = |gk| e_s + 3u |t|;   (tz + ty) + tx: + u |tz + ty| + u |total|
SAFETY = 2 is the one factor on top: it covers the second-order terms and an implementation that orders the same operations differently (torch's f32
evaluation of the module's tensor formula, which tests/test_bilateral_grid_ref_cpu.py holds to this budget on every case before any GPU run).  Nothing else
is added.

Budget maxima on the named case NAMED = 'lds' (grids (3, 12, 8, 4, 4), 96 x 200, idx 1; SAFETY included; `budget_maxima`; the CPU test asserts them below
the ceilings in brackets):
    out       8.78e-06 of max|out|        [2e-5]
    affine    7.61e-06 of max|A|          [2e-5]
    d_rgb     5.60e-06 of max|d_rgb|      [2e-5]
    d_grids   6.87e-05 of max|d_grids|    [2e-4]
i.e. 90 to 150 u of the tensor's scale for the per-pixel results: the coordinate error 2u c reaches 6u along x and y here (30u under 16 vertices) and
(L - 1) e_g = 7 e_g along z, and it enters every one of the 8 corner weights.  The d_grids figure is a sum's: d_out has random signs, so an entry that ~2 000
pixels touch is ~sqrt(2 000) times smaller than the sum of |addends| its 8 f32 additions are counted against.  torch's f32 evaluation of the tensor formula
uses 0.25 of this budget at the most (the ratios that tests/test_bilateral_grid_ref_cpu.py prints): worst-case counting against typical rounding.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
MARGIN = 1e-4
CR, CG, CB = (float(np.float32(v)) for v in (0.299, 0.587, 0.114))
COEF = np.array([CR, CG, CB])
NAMED = 'lds'
NAMED_CEILINGS = dict(out=2e-5, affine=2e-5, d_rgb=2e-5, d_grids=2e-4)


# ------------------------------------------------------------------------------------------------ the restatement
def _axis(t, n):
    """cell index, fraction and cell coordinate along an axis of n vertices."""
    if n == 1:
        return np.zeros(t.shape, np.int64), np.zeros(t.shape), np.zeros(t.shape)
    c = np.clip(t, 0.0, 1.0) * (n - 1)
    i = np.minimum(np.floor(c), n - 2).astype(np.int64)
    return i, c - i, c


def luminance_f32(rgb):
    """g by the kernel's f32 sequence (CR p0 + CG p1) + CB p2, as float64 numbers."""
    p = np.asarray(rgb, np.float32)
    c = np.float32
    return ((c(CR) * p[..., 0] + c(CG) * p[..., 1]) + c(CB) * p[..., 2]).astype(np.float64)


def _place(shape, rgb, g_f32):
    L, Gh, Gw = shape
    p = np.asarray(rgb, np.float64)
    H, W = p.shape[:2]
    u = np.broadcast_to(((np.arange(W) + 0.5) / W)[None, :], (H, W))
    v = np.broadcast_to(((np.arange(H) + 0.5) / H)[:, None], (H, W))
    g = luminance_f32(rgb) if g_f32 else (CR * p[..., 0] + CG * p[..., 1]) + CB * p[..., 2]
    return p, g, _axis(u, Gw), _axis(v, Gh), _axis(g, L)


def _corners(shape):
    L, Gh, Gw = shape
    return [(dz, dy, dx) for dy in range(2 if Gh > 1 else 1) for dx in range(2 if Gw > 1 else 1) for dz in range(2 if L > 1 else 1)]


def evaluate(grids, rgb, idx, d_out=None, g_f32=False):
    """float64.  grids (N, 12, L, Gh, Gw), rgb and d_out (H, W, 3).  Returns out (H, W, 3), affine (H, W, 12) and, with d_out, d_rgb (H, W, 3), d_grids (N, ...)."""
    grids = np.asarray(grids, np.float64)
    shape = grids.shape[2:]
    L = shape[0]
    p, g, (ix, fx, _), (iy, fy, _), (iz, fz, _) = _place(shape, rgb, g_f32)
    H, W = p.shape[:2]
    Gv = np.moveaxis(grids[idx], 0, -1)                                   # (L, Gh, Gw, 12)
    wsel = lambda f, d: f if d else 1.0 - f
    A = np.zeros((H, W, 12))
    for dz, dy, dx in _corners(shape):
        A += (wsel(fz, dz) * wsel(fy, dy) * wsel(fx, dx))[..., None] * Gv[iz + dz, iy + dy, ix + dx]
    q = np.concatenate([p, np.ones((H, W, 1))], -1)
    M = A.reshape(H, W, 3, 4)
    res = dict(out=(M * q[:, :, None, :]).sum(-1), affine=A)
    if d_out is None:
        return res
    d = np.asarray(d_out, np.float64)
    D = np.zeros((H, W, 12))
    if L > 1:
        for dz, dy, dx in _corners(shape):
            if dz == 0:
                D += (wsel(fy, dy) * wsel(fx, dx))[..., None] * (Gv[iz + 1, iy + dy, ix + dx] - Gv[iz, iy + dy, ix + dx])
    s = (D.reshape(H, W, 3, 4) * q[:, :, None, :]).sum(-1)
    gz = np.where((g >= 0.0) & (g <= 1.0), (d * s).sum(-1) * (L - 1), 0.0)
    res['d_rgb'] = np.einsum('hwr,hwrk->hwk', d, M[..., :3]) + COEF * gz[..., None]
    m = (d[..., :, None] * q[..., None, :]).reshape(H, W, 12)
    dG = np.zeros(Gv.shape)
    for dz, dy, dx in _corners(shape):
        np.add.at(dG, (iz + dz, iy + dy, ix + dx), (wsel(fz, dz) * wsel(fy, dy) * wsel(fx, dx))[..., None] * m)
    res['d_grids'] = np.zeros(grids.shape)
    res['d_grids'][idx] = np.moveaxis(dG, -1, 0)
    return res


def _diffs(grids):
    grids = np.asarray(grids, np.float64)
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        if n > 1:
            sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(5))
            yield axis, n, sl, grids[sl(1, n)] - grids[sl(0, n - 1)]


def tv(grids):
    """TV(G) = (1/N) sum_axis sum (G[i+1] - G[i])^2 / count_axis, float64."""
    N = np.asarray(grids).shape[0]
    return float(sum((d * d).sum() / (d.size / N) for _, _, _, d in _diffs(grids)) / N)


def tv_grad(grids, upstream=1.0):
    out = np.zeros(np.asarray(grids).shape)
    N = out.shape[0]
    for axis, n, sl, d in _diffs(grids):
        k = float(upstream) * 2.0 / d.size                                 # d.size = N count_axis
        out[sl(1, n)] += k * d
        out[sl(0, n - 1)] -= k * d
    return out


# ------------------------------------------------------------------------------------------------ the budget
def _axis_err(c, f, n):
    """(e_w0, e_w1) of the weights 1 - f and f along an axis of n vertices, for the x / y axes (e_c = 2u c)."""
    if n == 1:
        return np.zeros(c.shape), np.zeros(c.shape)
    e_f = 2 * U * c
    return e_f + U * (1.0 - f), e_f


def budget(grids, rgb, idx, d_out=None, g_f32=False):
    """Absolute error budgets (SAFETY included) for what `evaluate` returns.  The derivation is the module docstring's, line by line."""
    grids = np.asarray(grids, np.float64)
    shape = grids.shape[2:]
    L, Gh, Gw = shape
    u = U
    p, g, (ix, fx, cx), (iy, fy, cy), (iz, fz, cz) = _place(shape, rgb, g_f32)
    H, W = p.shape[:2]
    Gv = np.moveaxis(grids[idx], 0, -1)
    t0, t1, t2 = CR * p[..., 0], CG * p[..., 1], CB * p[..., 2]
    e_g = u * (np.abs(t0) + np.abs(t1) + np.abs(t2)) + u * np.abs(t0 + t1) + u * np.abs(g)
    ex, ey = _axis_err(cx, fx, Gw), _axis_err(cy, fy, Gh)
    if L > 1:
        e_fz = (L - 1) * e_g + u * cz
        ez = (e_fz + u * (1.0 - fz), e_fz)
    else:
        ez = (np.zeros((H, W)), np.zeros((H, W)))
    wsel = lambda f, d: f if d else 1.0 - f
    q = np.abs(np.concatenate([p, np.ones((H, W, 1))], -1))
    has_p = np.array([1.0, 1.0, 1.0, 0.0])                                  # the products with q_3 = 1 do not round
    e_A = np.zeros((H, W, 12))
    sum_A = np.zeros((H, W, 12))
    e_D = np.zeros((H, W, 12))
    sum_D = np.zeros((H, W, 12))
    corner_w = []
    for dz, dy, dx in _corners(shape):
        wy, wx, wz = wsel(fy, dy), wsel(fx, dx), wsel(fz, dz)
        wyx = wy * wx
        e_wyx = ey[dy] * wx + wy * ex[dx] + u * wyx
        w = wz * wyx
        e_w = ez[dz] * wyx + wz * e_wyx + u * w
        Gc = np.abs(Gv[iz + dz, iy + dy, ix + dx])
        e_A += e_w[..., None] * Gc + u * w[..., None] * Gc
        sum_A += w[..., None] * Gc
        corner_w.append(((dz, dy, dx), w, e_w))
        if dz == 0 and L > 1:
            dG = np.abs(Gv[iz + 1, iy + dy, ix + dx] - Gv[iz, iy + dy, ix + dx])
            e_D += e_wyx[..., None] * dG + 2 * u * wyx[..., None] * dG
            sum_D += wyx[..., None] * dG
    e_A += 7 * u * sum_A
    e_D += 3 * u * sum_D
    eA4 = e_A.reshape(H, W, 3, 4)
    M = evaluate(grids, rgb, idx, d_out, g_f32)
    A4 = np.abs(M['affine'].reshape(H, W, 3, 4))
    q4 = q[:, :, None, :]
    bud = dict(affine=e_A, out=(eA4 * q4).sum(-1) + u * (A4 * q4 * has_p).sum(-1) + 3 * u * (A4 * q4).sum(-1))
    if d_out is not None:
        d = np.abs(np.asarray(d_out, np.float64))
        dsg = np.asarray(d_out, np.float64)
        pq = np.concatenate([p, np.ones((H, W, 1))], -1)
        # D itself (signed) for |D q| and s
        Dm = np.zeros((H, W, 12))
        if L > 1:
            for dz, dy, dx in _corners(shape):
                if dz == 0:
                    Dm += (wsel(fy, dy) * wsel(fx, dx))[..., None] * (Gv[iz + 1, iy + dy, ix + dx] - Gv[iz, iy + dy, ix + dx])
        D4 = Dm.reshape(H, W, 3, 4)
        aDq = np.abs(D4) * q4
        s = (D4 * pq[:, :, None, :]).sum(-1)
        e_s = (e_D.reshape(H, W, 3, 4) * q4).sum(-1) + u * (aDq * has_p).sum(-1) + 3 * u * aDq.sum(-1)
        ds = np.abs(dsg * s)
        e_S = (d * e_s).sum(-1) + 3 * u * ds.sum(-1)
        inside = (g >= 0.0) & (g <= 1.0)
        gz = np.where(inside, (dsg * s).sum(-1) * (L - 1), 0.0)
        e_gz = np.where(inside, (L - 1) * e_S + u * np.abs(gz), 0.0)
        dA = d[..., :, None] * A4[..., :3]                                    # |d_r A_rk|
        e_lin = (d[..., :, None] * eA4[..., :3]).sum(-2) + 3 * u * dA.sum(-2)
        cg = COEF * gz[..., None]
        bud['d_rgb'] = e_lin + COEF * e_gz[..., None] + u * np.abs(cg) + u * np.abs(M['d_rgb'])
        m = (d[..., :, None] * q[..., None, :]).reshape(H, W, 12)
        e_m = u * m * np.tile(has_p, 3)
        eG = np.zeros(Gv.shape)
        for (dz, dy, dx), w, e_w in corner_w:
            v = w[..., None] * m
            np.add.at(eG, (iz + dz, iy + dy, ix + dx), e_w[..., None] * m + w[..., None] * e_m + u * v + 8 * u * v)
        bud['d_grids'] = np.zeros(grids.shape)
        bud['d_grids'][idx] = np.moveaxis(eG, -1, 0) + u * np.abs(M['d_grids'][idx])
    return {k: SAFETY * v for k, v in bud.items()}


def tv_budget(grids, upstream=1.0):
    """(budget of TV, budget array of its gradient), SAFETY included."""
    g = abs(float(upstream))
    e_grad = np.zeros(np.asarray(grids).shape)
    terms = []
    for axis, n, sl, d in _diffs(grids):
        gk = g * 2.0 / d.size
        d1 = np.zeros(e_grad.shape)
        d2 = np.zeros(e_grad.shape)
        d1[sl(1, n)] = d
        d2[sl(0, n - 1)] = d
        s = d1 - d2
        t = gk * s
        e_grad += gk * U * (np.abs(d1) + np.abs(d2) + np.abs(s)) + 3 * U * np.abs(t)
        terms.append(t)
    if terms:
        total = sum(terms)
        e_grad += U * np.abs(total)
        if len(terms) > 1:
            e_grad += U * np.abs(terms[0] + terms[1])
    return SAFETY * 3 * U * tv(grids), SAFETY * e_grad


def assert_within_budget(got, want, bud, what):
    """Every element: |got - want| <= budget.  Returns the largest error / budget ratio."""
    got, want, bud = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bud, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = np.where(err == 0, 0.0, err / np.where(bud > 0, bud, np.finfo(np.float64).tiny))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f'{what}: {int((ratio > 1).sum())} of {ratio.size} elements over budget, worst ratio {worst:.3f} (error {float(err.flat[ratio.argmax()]):.3e})'
    return worst


# ------------------------------------------------------------------------------------------------ inputs
def margins(shape, rgb, g_f32=False):
    """The smallest distance (in cells) of any c_x, c_y, c_z from an integer, and of g from 0 and 1 -- float64."""
    _, g, (_, _, cx), (_, _, cy), (_, _, cz) = _place(shape, rgb, g_f32)
    dist = lambda c, n: float(np.abs(c - np.round(c)).min()) if n > 1 else 1.0
    return min(dist(cx, shape[2]), dist(cy, shape[1]), dist(cz, shape[0])), float(np.minimum(np.abs(g), np.abs(g - 1.0)).min())


def _raw(n_grids, shape, H, W, seed):
    rng = np.random.default_rng(seed)
    grids = np.zeros((n_grids, 12) + tuple(shape), np.float32)
    grids[:, (0, 5, 10)] = 1.0
    grids += (0.2 * rng.standard_normal(grids.shape)).astype(np.float32)
    rgb = (0.02 + 0.96 * rng.random((H, W, 3))).astype(np.float32)
    d_out = rng.standard_normal((H, W, 3)).astype(np.float32)
    d_out[rng.random((H, W, 3)) < 0.2] = 0.0
    return grids, rgb, d_out


def draw(n_grids, shape, H, W, seed=7):
    """(grids, rgb (H, W, 3), d_out (H, W, 3)), f32, every pixel's c_z at least MARGIN from an integer and g from 0 and 1 (see the module docstring)."""
    grids, rgb, d_out = _raw(n_grids, shape, H, W, seed)
    for turn in range(1, 200):
        g = (CR * rgb[..., 0].astype(np.float64) + CG * rgb[..., 1]) + CB * rgb[..., 2]
        cz = np.clip(g, 0, 1) * (shape[0] - 1)
        bad = (np.minimum(np.abs(g), np.abs(g - 1.0)) < MARGIN)
        if shape[0] > 1:
            bad |= np.abs(cz - np.round(cz)) < MARGIN
        if not bad.any():
            return grids, rgb, d_out
        rgb = np.where(bad[..., None], _raw(1, (1, 1, 1), H, W, seed + 1000 * turn)[1], rgb)
    raise RuntimeError(f'no kink-free draw for {shape} on {H} x {W} from seed {seed}')


def _dyadic(rng, shape, step, span):
    return (rng.integers(-span, span + 1, shape) * step).astype(np.float32)


def exact(kind):
    """The named exact cases: (grids, rgb, d_out), dyadic.  'white', 'black', 'above' (p = 2), 'below' (p = -1): grids (1, 12, 3, 2, 2) on 4 x 5;
    'vertices': grids (1, 12, 3, 5, 9) on 2 x 4, the pixel centres on vertices along x and y, colours (0.5, 0, 0)-like so that the f32 luminance is exact."""
    rng = np.random.default_rng(11)
    if kind == 'vertices':
        grids = _dyadic(rng, (1, 12, 3, 5, 9), 0.125, 16)
        rgb = np.zeros((2, 4, 3), np.float32)
        rgb[..., 0] = np.array([[0.5, 1.0, 0.25, 2.0], [0.125, 0.5, 1.0, 0.25]], np.float32)
    else:
        grids = _dyadic(rng, (1, 12, 3, 2, 2), 0.125, 16)
        rgb = np.full((4, 5, 3), dict(white=1.0, black=0.0, above=2.0, below=-1.0)[kind], np.float32)
    d_out = _dyadic(rng, rgb.shape, 0.25, 8)
    return grids, rgb, d_out


EXACT = ('white', 'black', 'above', 'below', 'vertices')
# name: (number of grids, (L, Gh, Gw), H, W, idx, layout).  The smallest shapes at which each path can go wrong (32 x 8 pixel tiles, 64-lane waves, windows of
# at most 1536 floats in LDS): a global affine; one cell; several cells under one tile; tiles that span many cells (the direct path: 8 x 5 x-y vertices per
# tile); the LDS window path with tiles straddling cell borders, ragged image edges, N = 3 and several workgroups per grid entry; many workgroups; an axis of
# extent 1 between two others.  The x / y extents are even or 1: c = (2 x + 1) (n - 1) / (2 W) is then an odd number over an even one, never on a vertex.
CASES = {
    'affine': (1, (1, 1, 1), 5, 7, 0, 'hwc'),
    'cell': (1, (2, 2, 2), 3, 5, 0, 'chw'),
    'cells': (2, (3, 4, 6), 9, 11, 1, 'hwc'),
    'direct': (1, (8, 16, 16), 37, 70, 0, 'chw'),
    'lds': (3, (8, 4, 4), 96, 200, 1, 'hwc'),
    'many': (2, (8, 8, 8), 130, 330, 1, 'chw'),
    'flat_y': (1, (3, 1, 4), 10, 45, 0, 'chw'),
}
INTERIOR = ('cell', 'cells', 'direct', 'lds', 'flat_y')          # every extent a grid_sample can interpolate; 'flat_y' has one of 1 (grid_sample: size-1 axis)
TV_SHAPES = ((3, 12, 8, 16, 16), (2, 12, 1, 2, 5))
UPSTREAM = 0.625                                                    # exact in f32


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name in EXACT:
        return exact(name)
    n, shape, H, W, _, _ = CASES[name]
    return draw(n, shape, H, W)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(value dict, budget dict, idx, layout) of one case, computed once and shared; callers leave the arrays alone."""
    grids, rgb, d_out = inputs(name)
    idx, layout, g_f32 = (0, 'hwc', True) if name in EXACT else (*CASES[name][4:], False)
    return evaluate(grids, rgb, idx, d_out, g_f32), budget(grids, rgb, idx, d_out, g_f32), idx, layout


@functools.lru_cache(maxsize=None)
def tv_inputs(shape, kind='random'):
    rng = np.random.default_rng(5)
    if kind == 'constant':
        return np.full(shape, 0.375, np.float32)
    g = np.zeros(shape, np.float32)
    g[:, (0, 5, 10)] = 1.0
    return g + (0.2 * rng.standard_normal(shape)).astype(np.float32)


def identity_case():
    """An identity grid (1, 12, 4, 4, 4) on 9 x 11: (grids, rgb, d_out)."""
    _, rgb, d_out = draw(1, (4, 4, 4), 9, 11, seed=3)
    grids = np.zeros((1, 12, 4, 4, 4), np.float32)
    grids[:, (0, 5, 10)] = 1.0
    return grids, rgb, d_out


def budget_maxima(name=NAMED):
    val, bud, _, _ = reference(name)
    return {k: float(bud[k].max() / np.abs(val[k]).max()) for k in ('out', 'affine', 'd_rgb', 'd_grids')}


def to_layout(a, layout):
    """(H, W, 3) -> the case's layout."""
    return np.ascontiguousarray(np.moveaxis(a, -1, 0)) if layout == 'chw' else a


def from_layout(a, layout):
    return np.moveaxis(a, 0, -1) if layout == 'chw' else a
