"""Float64 statements, f32 restatements and per-element error budgets for the NeRF ray stages (nerficg_amd/csrc/nerf_rays.hip: k_nerf_sample_coarse,
k_nerf_integrate_fw / _bw, k_nerf_sample_fine; C ABI group 19, include/nerficg_hip.h; Python: nerficg_amd.nerf.sample_coarse / composite / sample_fine).
Plain module: no test functions.  Used by tests/test_nerf_rays_ref_cpu.py and tests/test_gpu_nerf_rays.py.

The f64 statements (`sample_coarse_f64`, `integrate_f64`, `integrate_backward_f64`, `sample_fine_f64`)
---------------------
The reference's formulas (src/Methods/NeRF/utils.py:57-136) in float64 on the given (f32) inputs; `integrate_backward_f64` is the closed form
    d_sigma_i = len_i (gw_i T_{i+1} - sum_{j>i} gw_j w_j - T_end B),   d_rgb_samples_i = w_i d_rgb,
    gw_i = d_rgb . c_i + d_weights_i,   B = d_rgb . background - d_alpha,
checked against torch f64 autograd through nerf.integrate_samples by the CPU tests.  `mut=` plants one of MUTATIONS.

The f32 restatements (`sample_coarse_f32`, `positions_f32`, `cdf_f32`, `fine_from_cdf_f32`, `sample_fine_f32`)
------------------------
numpy float32, one rounding per operation, in the order stated at the top of csrc/nerf_rays.hip (the file is built without FMA contraction): the device
must equal them BIT FOR BIT.  `cdf_f32` follows the device's summation order (lane chunks of ceil((Sc-2)/64) masses, a 6-step xor butterfly for the
total, the lanes' totals accumulated lane after lane); the GPU tests feed `fine_from_cdf_f32` the device's own cdf, so the bit-for-bit claim on the fine
depths does not rest on that order.

The budgets (u = 2^-24; every rounding of the stated sequence contributes u |value|, propagated by the f64 first-order sensitivities)
-----------
Compositing forward (`integrate_budget`), per ray, x_i = sigma_i len_i, e_i = exp(-x_i), a_i = 1 - e_i, m_i = 1 - a_i, T_i = prod_{j<i} m_j:
    x_i     delta (1 rounding), |d| (5 roundings under a square root + the root: <= 3.5 u), delta |d| (1), sigma len (1): <= 7 u relative, counted as 8;
    e_i     the argument's error enters as x_i 8 u RELATIVE; the accurate expf is within 1 ulp = 2 u:       eps_i = (8 x_i + 2) u  (+ 2^-126 absolute: the
            subnormal range may be flushed);
    a_i     d a_i = e_i eps_i + 2^-126 + min(u a_i, e_i)       (the rounding of 1 - e is at most half an ulp of a, and at most e itself once e < u);
    m_i     1 - a_i is exact for a_i >= 1/2 and one rounding otherwise: relative to e_i, rho_i = eps_i + min(u a_i / e_i, 1) + u (+ the floor).  rho_i can
            reach 1 on a saturated sample, so the product is bounded multiplicatively, not to first order:
    T_i     i + 1 multiplications (chunk product, scan, chunk walk: any tree over i factors, + the scan's seed):
            d T_i = T_i (exp(sum_{j<i} rho_j + (i + 2) u) - 1) + (i + 1) 2^-126;   T_end likewise with i = S;
    w_i     d w_i = u w_i + a_i d T_i + T_i d a_i;
    sums    a term passes at most D = ceil(S / 64) + 7 additions (its lane's partial sum, six butterfly steps, the closing one):
            d rgb_c = sum_i (|c_ic| d w_i + u w_i |c_ic|) + D u sum_i w_i |c_ic| + |bg_c| d T_end + u T_end |bg_c| + u |rgb_c|;
            d alpha = d T_end + u alpha;    d (sum w t) likewise;    d depth = d(sum w t) / alpha + |sum w t| d alpha / alpha^2 + u |depth| where T_end < 1,
            0 where T_end = 1 in f64 (every x_i is 0 then, and so it is in f32).
Compositing backward (`backward_budget`):
    gw_i    three products, two additions, + d_weights: 4 u (sum_c |g_c c_ic| + |d_weights_i|);   B likewise with the background and d_alpha;
    A_i = gw_i T_{i+1}:  u |A| + |gw| d T_{i+1} + T_{i+1} d gw;      g_j = gw_j w_j:  u |g_j| + |gw_j| d w_j + w_j d gw_j;
    S_i = sum_{j>i} g_j: sum_{j>i} d g_j + (ceil(S / 64) + 8) u sum_{j>i} |g_j|;      T_end B:  |B| d T_end + T_end d B + u |T_end B|;
    bracket = (A - S) - T_end B: the three + 2 u (|A| + |S| + |T_end B|);   len_i: 6 u len_i;   d_sigma_i: len d bracket + |bracket| d len + u |d_sigma_i|;
    d_rgb_samples_ic: |g_c| d w_i + u |w_i g_c|.
All budgets are multiplied by 1 + 2^-10 for the second-order terms (k u <= 2^-12 for every count k above).
CDF (`cdf_bound`):  |cdf_dev[k] - cdf_f64[k]| <= (2 Sc + 3) u cdf_f64[k]: the mass's rounding (1), the total's Sc additions, the division (1), k <= Sc
additions of positive terms, + 1.
Fine depths against the reference's f32 fixture (`fine_depth_budget`): (k1 - k0) 2 E_cdf / width_f64 + 4 u |t|, E_cdf = cdf_bound at the interval's right
end (the device's cdf and the fixture's each move by E_cdf), capped at the span of the sample's interval and its two neighbours.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
SECOND_ORDER = 1.0 + 2.0 ** -10
F32 = np.float32

MUTATIONS = ('strata_off_by_one', 'final_delta_unscaled', 'background_alpha', 'eps_all_masses', 'lower_bound', 'no_flat_rule', 'suffix_inclusive', 'T_i')


def _f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------------------------------- sampling
def _strata(t_row, mut=None):
    cuts = (t_row[1:] + t_row[:-1]) * t_row.dtype.type(0.5)
    lower, upper = np.concatenate((t_row[:1], cuts)), np.concatenate((cuts, t_row[-1:]))
    if mut == 'strata_off_by_one' and t_row.size > 1:      # the inner lower borders read cut_i instead of cut_{i-1}
        lower = np.concatenate((t_row[:1], cuts[1:], t_row[-1:]))
    return lower, upper


def sample_coarse_f64(t_row, u=None, n_rays=None, mut=None):
    t_row = _f64(t_row)
    if u is None:
        return np.broadcast_to(t_row, (n_rays, t_row.size)).copy()
    lower, upper = _strata(t_row, mut)
    return lower + (upper - lower) * _f64(u)


def sample_coarse_f32(t_row, u=None, n_rays=None, mut=None):
    t_row = np.asarray(t_row, F32)
    if u is None:
        return np.broadcast_to(t_row, (n_rays, t_row.size)).copy()
    lower, upper = _strata(t_row, mut)
    return (lower + (upper - lower) * np.asarray(u, F32)).astype(F32)


def positions_f32(origins, directions, t):
    o, d, t = np.asarray(origins, F32), np.asarray(directions, F32), np.asarray(t, F32)
    return (o[:, None, :] + d[:, None, :] * t[:, :, None]).astype(F32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------------------- compositing
def integrate_f64(t, directions, sigma, colors, background, final_delta, mut=None):
    """-> dict of rgb (N, 3), depth (N), alpha (N), weights (N, S) and the intermediates the budgets need"""
    t, d, sigma, c = _f64(t), _f64(directions), _f64(sigma).reshape(np.shape(t)), _f64(colors).reshape(*np.shape(t), 3)
    n, s = t.shape
    norm = np.sqrt((d * d).sum(-1))
    delta = np.concatenate((np.diff(t, axis=-1), np.full((n, 1), float(final_delta))), axis=-1)
    length = delta * norm[:, None]
    if mut == 'final_delta_unscaled':
        length[:, -1] = float(final_delta)
    with np.errstate(over='ignore', under='ignore'):
        x = sigma * length
        e = np.exp(-x)
        a = -np.expm1(-x)
    t_incl = np.cumprod(e, axis=-1)
    T = np.concatenate((np.ones((n, 1)), t_incl[:, :-1]), axis=-1)
    t_end = t_incl[:, -1]
    w = a * T
    rgb = (w[:, :, None] * c).sum(1)
    if background is not None:
        rgb = rgb + ((1.0 - t_end) if mut == 'background_alpha' else t_end)[:, None] * _f64(background)[None, :]
    alpha = 1.0 - t_end
    wt = (w * t).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        depth = np.where(t_end < 1.0, wt / alpha, 0.0)
    return dict(rgb=rgb, depth=depth, alpha=alpha, weights=w, T=T, T_end=t_end, e=e, a=a, x=x, length=length, wt=wt, t=t, c=c,
                bg=None if background is None else _f64(background))


def _upstream(n, s, d_rgb, d_alpha, d_weights):
    g = np.zeros((n, 3)) if d_rgb is None else _f64(d_rgb).reshape(n, 3)
    da = np.zeros(n) if d_alpha is None else _f64(d_alpha).reshape(n)
    dw = np.zeros((n, s)) if d_weights is None else _f64(d_weights).reshape(n, s)
    return g, da, dw


def integrate_backward_f64(fw, d_rgb, d_alpha, d_weights, mut=None):
    """fw: the dict of integrate_f64 -> (d_sigma (N, S), d_rgb_samples (N, S, 3)) and the intermediates"""
    w, T, e, c = fw['weights'], fw['T'], fw['e'], fw['c']
    n, s = w.shape
    g, da, dw = _upstream(n, s, d_rgb, d_alpha, d_weights)
    gw = (g[:, None, :] * c).sum(-1) + dw
    B = (0.0 if fw['bg'] is None else (g * fw['bg'][None, :]).sum(-1)) - da
    T1 = T if mut == 'T_i' else T * e
    gj = gw * w
    rev = np.cumsum(gj[:, ::-1], axis=-1)[:, ::-1]          # inclusive suffix sums
    suffix = rev if mut == 'suffix_inclusive' else np.concatenate((rev[:, 1:], np.zeros((n, 1))), axis=-1)
    A, TB = gw * T1, fw['T_end'] * B
    bracket = A - suffix - TB[:, None]
    d_sigma = fw['length'] * bracket
    return d_sigma, w[:, :, None] * g[:, None, :], dict(gw=gw, B=B, A=A, TB=TB, suffix=suffix, gj=gj, g=g, da=da, dw=dw, bracket=bracket)


def _forward_errors(fw):
    x, e, a, T, w = fw['x'], fw['e'], fw['a'], fw['T'], fw['weights']
    n, s = w.shape
    eps = (8.0 * x + 2.0) * U
    d_a = e * eps + FLOOR + np.minimum(U * a, e)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        rho = np.where(e > 0.0, eps + np.minimum(U * a / e, 1.0) + U, 1.0)
    rho = np.where(np.isfinite(rho), rho, 1.0)
    cum = np.concatenate((np.zeros((n, 1)), np.cumsum(rho, axis=-1)), axis=-1)            # cum[:, i] = sum_{j<i} rho_j, i = 0 .. S
    idx = np.arange(s + 1)[None, :]
    with np.errstate(over='ignore'):
        grow = np.expm1(np.minimum(cum + (idx + 2) * U, 700.0))
    t_all = np.concatenate((T, fw['T_end'][:, None]), axis=-1)
    d_t_all = t_all * grow + (idx + 1) * FLOOR
    d_T, d_T_end, d_T1 = d_t_all[:, :-1], d_t_all[:, -1], d_t_all[:, 1:]
    d_w = U * w + a * d_T + T * d_a
    return d_a, d_T, d_T1, d_T_end, d_w


def integrate_budget(fw, sum_depth=None):
    """-> dict of per-element bounds on |device - f64| for rgb (N, 3), depth (N), alpha (N), weights (N, S).  sum_depth: additions a term of the three
    sums passes; None = the device's ceil(S / 64) + 7, S + 1 = the worst case of ANY summation order (an f32 implementation that sums otherwise)."""
    w, c, t, t_end = fw['weights'], fw['c'], fw['t'], fw['T_end']
    n, s = w.shape
    _, _, _, d_T_end, d_w = _forward_errors(fw)
    D = -(-s // 64) + 7 if sum_depth is None else sum_depth
    ac = np.abs(c)
    rgb = (d_w[:, :, None] * ac + U * w[:, :, None] * ac).sum(1) + D * U * (w[:, :, None] * ac).sum(1) + U * np.abs(fw['rgb'])
    if fw['bg'] is not None:
        rgb = rgb + np.abs(fw['bg'])[None, :] * (d_T_end + U * t_end)[:, None]
    alpha = d_T_end + U * fw['alpha']
    d_wt = (d_w * np.abs(t) + U * w * np.abs(t)).sum(-1) + D * U * (w * np.abs(t)).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        depth = np.where(t_end < 1.0, d_wt / fw['alpha'] + np.abs(fw['wt']) * alpha / fw['alpha'] ** 2 + U * np.abs(fw['depth']), 0.0)
    return {k: v * SECOND_ORDER for k, v in dict(rgb=rgb, depth=depth, alpha=alpha, weights=d_w).items()}


def backward_budget(fw, bw):
    """fw: integrate_f64's dict, bw: the third value of integrate_backward_f64 -> (bound on d_sigma (N, S), bound on d_rgb_samples (N, S, 3))"""
    w, c, T, e = fw['weights'], fw['c'], fw['T'], fw['e']
    n, s = w.shape
    _, _, d_T1, d_T_end, d_w = _forward_errors(fw)
    g, gw, B, A, TB, gj, suffix = bw['g'], bw['gw'], bw['B'], bw['A'], bw['TB'], bw['gj'], bw['suffix']
    d_gw = 4.0 * U * ((np.abs(g)[:, None, :] * np.abs(c)).sum(-1) + np.abs(bw['dw']))
    T1 = T * e
    d_A = U * np.abs(A) + np.abs(gw) * d_T1 + T1 * d_gw
    d_gj = U * np.abs(gj) + np.abs(gw) * d_w + w * d_gw

    def after(v):      # sum over j > i
        rev = np.cumsum(v[:, ::-1], axis=-1)[:, ::-1]
        return np.concatenate((rev[:, 1:], np.zeros((n, 1))), axis=-1)
    abs_suffix = after(np.abs(gj))
    d_S = after(d_gj) + (-(-s // 64) + 8) * U * abs_suffix
    d_B = 4.0 * U * ((0.0 if fw['bg'] is None else (np.abs(g) * np.abs(fw['bg'])[None, :]).sum(-1)) + np.abs(bw['da']))
    d_TB = np.abs(B) * d_T_end + fw['T_end'] * d_B + U * np.abs(TB)
    d_br = d_A + d_S + d_TB[:, None] + 2.0 * U * (np.abs(A) + abs_suffix + np.abs(TB)[:, None])
    length = np.abs(fw['length'])
    d_sigma = length * d_br + np.abs(bw['bracket']) * 6.0 * U * length + U * np.abs(length * bw['bracket'])
    d_samples = np.abs(g)[:, None, :] * d_w[:, :, None] + U * np.abs(w[:, :, None] * g[:, None, :])
    return d_sigma * SECOND_ORDER, d_samples * SECOND_ORDER


# ------------------------------------------------------------------------------------------------------------------------------- resampling
def knots_of(t_coarse):
    b = np.asarray(t_coarse)
    return (b[:, 1:] + b[:, :-1]) * b.dtype.type(0.5)


def cdf_f64(weights, mut=None):
    w = _f64(weights)
    mass = w[:, 1:-1] + 1e-5
    total = (w + 1e-5).sum(-1, keepdims=True) if mut == 'eps_all_masses' else mass.sum(-1, keepdims=True)
    return np.concatenate((np.zeros((w.shape[0], 1)), np.cumsum(mass / total, axis=-1)), axis=-1)


def cdf_f32(weights, mut=None):
    """The device's f32 sequence and summation order -> (N, Sc - 1) float32"""
    w = np.asarray(weights, F32)
    n, sc = w.shape
    m = sc - 2
    cm = -(-m // 64)
    mass = np.zeros((n, 64 * cm), F32)
    mass[:, :m] = w[:, 1:-1] + F32(1e-5)
    chunks = mass.reshape(n, 64, cm)
    part = np.zeros((n, 64), F32)
    for k in range(cm):
        part = part + chunks[:, :, k]
    lanes = np.arange(64)
    v = part
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ d]
    total = v[:, :1]
    if mut == 'eps_all_masses':
        total = total + ((w[:, :1] + F32(1e-5)) + (w[:, -1:] + F32(1e-5)))
    run = np.zeros((n, 64), F32)
    local = np.zeros((n, 64, cm), F32)
    for k in range(cm):
        run = run + chunks[:, :, k] / total
        local[:, :, k] = run
    prefix = np.zeros((n, 64), F32)
    acc = np.zeros(n, F32)
    for l in range(64):
        prefix[:, l] = acc
        acc = acc + run[:, l]
    out = (prefix[:, :, None] + local).reshape(n, 64 * cm)[:, :m]
    return np.concatenate((np.zeros((n, 1), F32), out), axis=-1).astype(F32)


def cdf_bound(cdf64, n_coarse):
    return (2 * n_coarse + 3) * U * _f64(cdf64)


def _invert(knots, cdf, u, mut=None):
    """dtype-generic: knots, cdf (N, K), u (N, Sf) -> t_fine (N, Sf) and the two indices"""
    n, k = cdf.shape
    side = 'left' if mut == 'lower_bound' else 'right'
    right = np.stack([np.searchsorted(cdf[r], u[r], side=side) for r in range(n)])
    left = np.maximum(right - 1, 0)
    right = np.minimum(right, k - 1)
    c0, c1 = np.take_along_axis(cdf, left, 1), np.take_along_axis(cdf, right, 1)
    k0, k1 = np.take_along_axis(knots, left, 1), np.take_along_axis(knots, right, 1)
    width = c1 - c0
    if mut != 'no_flat_rule':
        width = np.where(width < cdf.dtype.type(1e-5), cdf.dtype.type(1.0), width)
    with np.errstate(divide='ignore', invalid='ignore'):
        return k0 + ((u - c0) / width) * (k1 - k0), left, right


def _rows_of_u(u, n, dtype):
    u = np.asarray(u, dtype)
    return np.ascontiguousarray(np.broadcast_to(u, (n, u.shape[-1])))


def fine_from_cdf_f32(t_coarse, cdf, u, mut=None):
    """t_fine (N, Sf) float32 from a given f32 cdf (the device's own, in the GPU tests), in the order of u"""
    tc = np.asarray(t_coarse, F32)
    out, _, _ = _invert(knots_of(tc), np.asarray(cdf, F32), _rows_of_u(u, tc.shape[0], F32), mut)
    return out.astype(F32)


def sample_fine_f32(t_coarse, weights, u, mut=None):
    """-> (t (N, Sc + Sf) ascending, t_fine (N, Sf), cdf (N, Sc - 1)), all float32"""
    cdf = cdf_f32(weights, 'eps_all_masses' if mut == 'eps_all_masses' else None)
    t_fine = fine_from_cdf_f32(t_coarse, cdf, u, mut)
    return np.sort(np.concatenate((np.asarray(t_coarse, F32), t_fine), axis=-1), axis=-1), t_fine, cdf


def sample_fine_f64(t_coarse, weights, u, mut=None):
    """-> (t_fine (N, Sf), cdf (N, Sc - 1), left index, right index) in float64"""
    tc = _f64(t_coarse)
    cdf = cdf_f64(weights, mut)
    out, left, right = _invert(knots_of(tc), cdf, _rows_of_u(u, tc.shape[0], np.float64), mut)
    return out, cdf, left, right


def fine_depth_budget(t_coarse, weights, u):
    """Per-sample bound on |f32 implementation - f32 reference fixture| (module docstring) and the smallest f64 interval width that a sample uses"""
    tc = _f64(t_coarse)
    n, sc = tc.shape
    t64, cdf, left, right = sample_fine_f64(tc, weights, u)
    knots = knots_of(tc)
    c0, c1 = np.take_along_axis(cdf, left, 1), np.take_along_axis(cdf, right, 1)
    k0, k1 = np.take_along_axis(knots, left, 1), np.take_along_axis(knots, right, 1)
    width = c1 - c0
    e_cdf = cdf_bound(c1, sc)
    with np.errstate(divide='ignore', invalid='ignore'):
        bound = np.where(width > 0.0, (k1 - k0) * 2.0 * e_cdf / width, np.inf) + 4.0 * U * np.abs(t64)
    lo, hi = np.maximum(left - 1, 0), np.minimum(right + 1, sc - 2)
    span = np.take_along_axis(knots, hi, 1) - np.take_along_axis(knots, lo, 1)
    return np.minimum(bound, span + 4.0 * U * np.abs(t64)), float(np.where(right > left, width, np.inf).min())


def judge(name, got, want, bound):
    """max of |got - want| / bound over the elements (0 / 0 = 0); raises AssertionError naming the worst element when it exceeds 1"""
    got, want, bound = _f64(got), _f64(want), _f64(bound)
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), f'{name}: non-finite values'
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        at = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
        raise AssertionError(f'{name}: element {at} is off by {err[at]:.3e}, its budget is {bound[at]:.3e} (got {got[at]!r}, want {want[at]!r})')
    return worst
