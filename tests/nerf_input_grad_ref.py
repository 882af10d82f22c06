"""A float64 restatement, an exactness proof and per-element error budgets for the vanilla NeRF path's gradients to its INPUTS (C ABI group 20,
include/nerficg_hip.h): the block's input gradient (nerficg_amd/csrc/nerf_input_grad.hip: k_nerf_input_grad, k_nerf_dir_reduce) and the two ray stages
(nerficg_amd/csrc/nerf_rays.hip: k_nerf_positions_bw, k_nerf_integrate_bw<true>); Python: nerficg_amd.nerf.fused_apply / sample_coarse / sample_fine /
composite / render_rays with input_grad=True.  Plain module: no test functions.  The block's restatement, its net containers and judges come from
tests/nerf_mlp_ref.py (R) and tests/nerf_grad_ref.py (B), the compositor's from tests/nerf_rays_ref.py (Y): read their docstrings first.  Used by
tests/test_nerf_input_grad_ref_cpu.py and tests/test_gpu_nerf_input_grad.py.

The restatement (`enc_gradients`, `encoding_backward`, `input_gradients`)
---------------
G[.] are the gradient stages of the backward (B.backward, or the device's through nrc_nerf_grad_stage), scaled by S = 2^e; W16 = sat(h16(W)).
    dE_pos[m, i] = sum_o W16_0[o, i] G[H_1][m, o] + sum_{k in skips, ascending} sum_o W16_k[o, W + i] G[H_k+1][m, o]
    dE_dir[m, j] = sum_o W16_colour[o, W + j] G[C_1][m, o]
fp16 operands, one f32 accumulator per output starting at 0, no fp16 conversion, no saturation, no mask.  Encoding backward, per row and component c,
a_k = x_c 2^k (exact), (s_k, c_k) = (sin a_k, cos a_k) -- float64 here, the forward's own nerf_sincos on the device:
    dx_c = [append] dE[c] + sum_{k<K} 2^k (c_k dE[sin_c,k] - s_k dE[cos_c,k]),    columns: cos at 3 append + 2 K c + k, sin at + K,
then one multiplication by 2^-e.  d_positions = dx of the position; the per-row direction gradient likewise, and d_directions[g] = its sum over the
rows g dir_group .. min((g + 1) dir_group, M) - 1.  The device's summation order (each lane half its columns in ascending order, half 0 + half 1; the group
sum lane-strided, then a butterfly) is stated in csrc/nerf_input_grad.hip; no budget below depends on it.
`rounding=False` uses the weights as given and expects unrounded stages (B.backward(rounding=False)): the plain chain rule, which the CPU tests hold
against float64 torch autograd through an f64 NeRFBlock.

Exactness (`exact`)
-------------------
As in B.exact: if every accumulator's sum of |addends| stays below 2^24 units (the unit a power of two dividing every addend), no partial sum in any
order rounds in f32 and the device equals the restatement bit for bit.  With K = 0 and append_input the encoding is the identity (dx = dE); with x = 0
and K = 10 / 4 nerf_sincos returns cos = 1 and sin = 0 exactly (the forward's exact cases rely on the same), so dx_c = sum_k 2^k dE[sin_c,k].  The nets are
B.exact_net (the recipe of R.exact_net with the one colour layer the training path supports) and R.exact_net(., 'zero'); the upstream is B.exact_upstream.

The budgets (u = 2^-24, gamma(k) = k u / (1 - k u), E_ENC = 2^-22 from tests/nerf_mlp_ref.py: |x| <= 8, k <= 9)
-----------
One stage at a time, from what the DEVICE produced in front of it:
    dE:       |device - Z| <= gamma(n_terms + 2) sum |W16| |G|, G the device's stages; n_terms = W (1 + number of skips) for the position, W / 2 for the
              direction.
    dx:       from the device's dE:  |device - z 2^-e| <= (gamma(2 K + 3) A + E_ENC sum_k 2^k (|dE_sin| + |dE_cos|)) 2^-e + 2^-149, A the sum of |addends|:
              an addend passes one product and at most 2 K + 1 additions (2 K + 1 addends per component, any order); the scaling by 2^k and by 2^-e is
              exact unless the result is subnormal (the last term); sin / cos are within E_ENC of the float64 functions.
    grouped:  the device's per-row values (a run with dir_group = 1, bit-identical to what the grouped run sums):
              |device - f64 sum| <= (n + 2) u sum |addends|, n the rows of the group.
    positions_backward:  d_o = sum_s g_s, d_d = sum_s t_s g_s:  (S + 2) u sum |addends| per element (one product, at most S - 1 additions).
    the |d| term of the compositor (`dirs_term_f64`, `dirs_budget`):  with q_i the bracket of Y.integrate_backward_f64 (d_sigma_i = len_i q_i),
              p_i = q_i sigma_i Delta_i, P = sum_i p_i, d_directions = (d / |d|) P.  Y.backward_budget bounds d_sigma_i by len_i dq_i + 7 u |len_i q_i|
              (dq_i its bound on the bracket, which it does not return), so dq_i <= bound(d_sigma_i) / len_i where len_i > 0 -- the same propagated
              roundings that give d_sigma its budget.  Then  d p_i = sigma_i Delta_i dq_i + 3 u |p_i|  (Delta: one subtraction, sigma Delta: one product,
              q (sigma Delta): one product),  d P = sum_i d p_i + D u sum_i |p_i| with D = ceil(S / 64) + 7 additions on a term's path as in Y's sums, and
              d / |d|: the norm (<= 3.5 u, counted 4), the division and the closing product: 6 u |result|:
              bound_c = (|d_c| / |d|) d P + 6 u |d_directions_c|, times Y.SECOND_ORDER.  Where |d| = 0 the device must return 0.
              The reference of the GPU test is float64 torch autograd through nerf.integrate_samples; the CPU tests hold `dirs_term_f64` against it.
No measured constant, no tensor maximum and no excluded element enters.
"""
from __future__ import annotations

import numpy as np

from tests import nerf_grad_ref as B
from tests import nerf_mlp_ref as R
from tests import nerf_rays_ref as Y
from tests.nerf_mlp_ref import E_ENC, gamma32, h16, sat, judge  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
TINY = 2.0 ** -149

MUTATIONS = ('swap_derivatives', 'cos_sign', 'no_pow2', 'drop_skip', 'skip_wrong_stage', 'drop_append', 'dir_in_front', 'no_unscale')
RAY_MUTATIONS = ('origin_weighted', 'direction_unweighted', 'dirs_final_delta_dropped', 'dirs_not_normalised', 'dirs_length_twice')


def _w(net, li, rounding=True):
    return sat(h16(net['lin'][li][0])) if rounding else np.asarray(net['lin'][li][0], np.float64)


# ------------------------------------------------------------------------------------------------ the restatement
def pos_parts(net, mut=None, rounding=True):
    """[(weight columns (W, n_pos), name of the gradient stage)] in the order the accumulator takes them"""
    W, n_pos = net['width'], R.n_enc(net['k_pos'], net['append'])
    parts = [(_w(net, 0, rounding), 'H_1')]
    if mut != 'drop_skip':
        for k in sorted(net['skips']):
            parts.append((_w(net, k, rounding)[:, W:W + n_pos], f'H_{k}' if mut == 'skip_wrong_stage' else f'H_{k + 1}'))
    return parts


def dir_part(net, mut=None, rounding=True):
    W, n_dir = net['width'], R.n_enc(net['k_dir'], net['append'])
    w = _w(net, net['L'] + 2, rounding)
    return [(w[:, :n_dir] if mut == 'dir_in_front' else w[:, W:W + n_dir], 'C_1')]


def _accumulate(parts, G):
    Z, A, n = 0.0, 0.0, 0
    for w, gname in parts:
        g = np.asarray(G[gname], np.float64)
        Z, A, n = Z + g @ w, A + np.abs(g) @ np.abs(w), n + g.shape[1]
    return dict(Z=Z, abs=A, n_terms=n)


def enc_gradients(net, G, mut=None, rounding=True):
    """-> dict(pos=dict(Z (M, n_pos), abs, n_terms), dir=dict(Z (M, n_dir), abs, n_terms)), still scaled by S"""
    return dict(pos=_accumulate(pos_parts(net, mut, rounding), G), dir=_accumulate(dir_part(net, mut, rounding), G))


def encoding_backward(x, dE, K, append, mut=None):
    """x (M, 3) f32 numbers, dE (M, 6 K + 3 append) -> dict(z (M, 3), abs (M, 3): the sum of |addends|, trig (M, 3): sum_k 2^k (|dE_sin| + |dE_cos|))"""
    x, dE = np.asarray(x, np.float32).astype(np.float64), np.asarray(dE, np.float64)
    m, a = x.shape[0], 3 if append else 0
    z, A, T = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3))
    if append and mut != 'drop_append':
        z, A = z + dE[:, :3], A + np.abs(dE[:, :3])
    for c in range(3):
        for k in range(K):
            p2 = 1.0 if mut == 'no_pow2' else 2.0 ** k
            arg = x[:, c] * 2.0 ** k
            s, co = np.sin(arg), np.cos(arg)
            d_cos, d_sin = dE[:, a + 2 * K * c + k], dE[:, a + 2 * K * c + K + k]
            if mut == 'swap_derivatives':
                d_cos, d_sin = d_sin, d_cos
            t_sin, t_cos = p2 * co * d_sin, (p2 if mut == 'cos_sign' else -p2) * s * d_cos
            z[:, c] += t_sin + t_cos
            A[:, c] += np.abs(t_sin) + np.abs(t_cos)
            T[:, c] += 2.0 ** k * (np.abs(d_sin) + np.abs(d_cos))
    return dict(z=z, abs=A, trig=T)


def row_directions(directions, m, dir_group):
    return np.asarray(directions, np.float32)[np.arange(m) // int(dir_group)]


def group_sums(rows, dir_group):
    """(sums (ceil(M / dir_group), 3), sums of |addends|, rows per group) of per-row values (M, 3) in float64"""
    rows = np.asarray(rows, np.float64)
    m, g = rows.shape[0], int(dir_group)
    n = -(-m // g)
    pad = np.zeros((n * g, 3))
    pad[:m] = rows
    count = np.minimum(g, m - g * np.arange(n))
    return pad.reshape(n, g, 3).sum(1), np.abs(pad).reshape(n, g, 3).sum(1), count


def input_gradients(net, G, positions, directions, S, dir_group=1, mut=None, rounding=True):
    """-> dict(dE_pos, dE_dir (scaled by S), d_positions (M, 3), dir_rows (M, 3), d_directions (ceil(M / dir_group), 3)).  mut: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS
    m = np.asarray(positions).shape[0]
    e = enc_gradients(net, G, mut, rounding)
    inv = 1.0 if mut == 'no_unscale' else 1.0 / S
    dp = encoding_backward(positions, e['pos']['Z'], net['k_pos'], net['append'], mut)['z'] * inv
    dd = encoding_backward(row_directions(directions, m, dir_group), e['dir']['Z'], net['k_dir'], net['append'], mut)['z'] * inv
    return dict(dE_pos=e['pos']['Z'], dE_dir=e['dir']['Z'], d_positions=dp, dir_rows=dd, d_directions=group_sums(dd, dir_group)[0])


# ------------------------------------------------------------------------------------------------ exactness
def _units_ok(addends):
    """every row's sum of |addends| below 2^24 units, the unit the lowest set bit among the row's addends"""
    a = np.asarray(addends, np.float64)
    bits = R._bits(a)
    unit = R._low(np.bitwise_or.reduce(bits, axis=-1))
    s = np.abs(a).sum(-1)
    return bool(np.all(np.where(s > 0, s / (2.0 ** 24 * np.where(np.isfinite(unit), unit, 1.0)), 0.0) < 1.0))


def exact(net, G, positions, directions, S, dir_group=1):
    """True when the device must equal `input_gradients` bit for bit: the encoding is the identity or the inputs are 0, every dE accumulator, every dx
    sum and every group sum stays below 2^24 units, and every result is an f32 number."""
    pos, dirs = np.asarray(positions, np.float64), np.asarray(directions, np.float64)
    ok = (net['k_pos'] == 0 or not pos.any()) and (net['k_dir'] == 0 or not dirs.any())
    ratios = [R._acc_ratio(np.asarray(G[g], np.float64), w, np.zeros(w.shape[1])) for w, g in pos_parts(net) + dir_part(net)]
    ok = ok and max(ratios) < 1.0
    out = input_gradients(net, G, positions, directions, S, dir_group)
    a = 3 if net['append'] else 0
    for dE, K in ((out['dE_pos'], net['k_pos']), (out['dE_dir'], net['k_dir'])):
        for c in range(3):
            cols = ([c] if a else []) + [a + 2 * K * c + K + k for k in range(K)]
            ok = ok and _units_ok(dE[:, cols] * np.array(([1.0] if a else []) + [2.0 ** k for k in range(K)])[None, :])
    g = int(dir_group)
    m = out['dir_rows'].shape[0]
    pad = np.zeros((-(-m // g) * g, 3))
    pad[:m] = out['dir_rows']
    ok = ok and _units_ok(pad.reshape(-1, g, 3).transpose(0, 2, 1))
    for k in ('d_positions', 'd_directions', 'dE_pos', 'dE_dir'):
        ok = ok and bool(np.array_equal(out[k].astype(np.float32).astype(np.float64), out[k]))
    return bool(ok)


def exact_check(ref, got):
    """names of the outputs of `got` that differ from the restatement `ref` of an exact case, bit for bit"""
    return [k for k in ('dE_pos', 'dE_dir', 'd_positions', 'dir_rows', 'd_directions')
            if k in got and not np.array_equal(np.asarray(got[k], np.float64).reshape(ref[k].shape), ref[k])]


# ------------------------------------------------------------------------------------------------ budgets
def enc_budget(net, G):
    """{'pos': (Z, bound), 'dir': (Z, bound)} from the gradient stages in G (the device's own)"""
    e = enc_gradients(net, G)
    return {k: (v['Z'], gamma32(v['n_terms'] + 2) * v['abs']) for k, v in e.items()}


def dx_budget(x, dE, K, append, e):
    """(ref, bound) of the unscaled input gradient from the encoded-input gradient dE (the device's own, scaled by 2^e)"""
    eb = encoding_backward(x, dE, K, append)
    inv = 2.0 ** -int(e)
    return eb['z'] * inv, (gamma32(2 * K + 3) * eb['abs'] + E_ENC * eb['trig']) * inv + TINY


def group_budget(rows, dir_group):
    """(ref, bound) of the grouped direction gradient from the per-row values (the device's own, dir_group = 1)"""
    s, a, n = group_sums(rows, dir_group)
    return s, (n[:, None] + 2) * U * a


def group_sums_f32(rows, dir_group):
    """The device's f32 sequence for the grouped direction gradient: lane l of 64 adds rows l, l + 64, .. of the group in ascending order starting at 0,
    then a butterfly over the lanes (distances 32 .. 1).  The GPU tests feed it the per-row values of a dir_group = 1 run: equality bit for bit says that
    those are the values the grouped run sums."""
    rows = np.asarray(rows, np.float32)
    m, g = rows.shape[0], int(dir_group)
    n, c = -(-m // g), -(-g // 64)
    pad = np.zeros((n, 64 * c, 3), np.float32)
    for k in range(n):
        r = rows[k * g:min((k + 1) * g, m)]
        pad[k, :r.shape[0]] = r
    part = np.zeros((n, 64, 3), np.float32)
    for j in range(c):
        part = part + pad[:, 64 * j:64 * (j + 1)]
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ d]
    return part[:, 0].astype(np.float64)


def chained_check(net, G, positions, directions, e, dir_group, got, rows=None):
    """Every output of `got` (a device's, or a mutant restatement's) against the restatement applied to what stands in front of it: dE from G, dx from
    got's own dE, the grouped directions from `rows` (default: got's own per-row values).  -> {name: (elements over their bound, worst error / bound)}"""
    res = {}
    m = np.asarray(positions).shape[0]
    eb = enc_budget(net, G)
    for name, key in (('dE_pos', 'pos'), ('dE_dir', 'dir')):
        ratio, over = judge(np.asarray(got[name], np.float64), *eb[key])
        res[name] = (over, ratio)
    ref, bound = dx_budget(positions, got['dE_pos'], net['k_pos'], net['append'], e)
    ratio, over = judge(np.asarray(got['d_positions'], np.float64), ref, bound)
    res['d_positions'] = (over, ratio)
    ref, bound = dx_budget(row_directions(directions, m, dir_group), got['dE_dir'], net['k_dir'], net['append'], e)
    ratio, over = judge(np.asarray(got['dir_rows'], np.float64), ref, bound)
    res['dir_rows'] = (over, ratio)
    ref, bound = group_budget(got['dir_rows'] if rows is None else rows, dir_group)
    ratio, over = judge(np.asarray(got['d_directions'], np.float64), ref, bound)
    res['d_directions'] = (over, ratio)
    return res


def dx_f32_model(x, dE, K, append, e):
    """An f32 emulation of the encoding backward with the forward's own sin / cos (R.sincos_model): every product and every addition rounded to f32, the
    addends of a component in ascending column order.  What a device with that order returns; the budget must hold it."""
    f32 = np.float32
    x, dE = np.asarray(x, f32), np.asarray(dE, f32)
    a = 3 if append else 0
    out = np.zeros((x.shape[0], 3), f32)
    for c in range(3):
        acc = np.zeros(x.shape[0], f32)
        if append:
            acc = (acc + dE[:, c]).astype(f32)
        for is_sin in (0, 1):
            for k in range(K):
                p2 = f32(2.0 ** k)
                sn, cs = R.sincos_model((x[:, c] * p2).astype(f32))
                v = dE[:, a + 2 * K * c + K * is_sin + k]
                term = (p2 * ((cs.astype(f32) * v).astype(f32) if is_sin else -(sn.astype(f32) * v).astype(f32))).astype(f32)
                acc = (acc + term).astype(f32)
        out[:, c] = (acc * f32(2.0 ** -int(e))).astype(f32)
    return out.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the ray stages
def positions_backward_f64(d_positions, t, mut=None):
    """the backward of positions = o + d t -> (d_origins (N, 3), d_directions (N, 3), their sums of |addends|)"""
    t = np.asarray(t, np.float64)
    n, s = t.shape
    g = np.asarray(d_positions, np.float64).reshape(n, s, 3)
    wo = t[:, :, None] if mut == 'origin_weighted' else 1.0
    wd = 1.0 if mut == 'direction_unweighted' else t[:, :, None]
    return (g * wo).sum(1), (g * wd).sum(1), np.abs(g * wo).sum(1), np.abs(g * wd).sum(1)


def positions_backward_budget(d_positions, t):
    """((d_origins, bound), (d_directions, bound))"""
    d_o, d_d, a_o, a_d = positions_backward_f64(d_positions, t)
    s = np.asarray(t).shape[1]
    return (d_o, (s + 2) * U * a_o), (d_d, (s + 2) * U * a_d)


def dirs_term_f64(fw, aux, directions, sigma, final_delta, mut=None):
    """fw: Y.integrate_f64's dict, aux: the third value of Y.integrate_backward_f64 -> (d_directions (N, 3), p (N, S)): the gradient through |d| in the
    segment lengths.  mut: one of RAY_MUTATIONS[2:]."""
    t, d = fw['t'], np.asarray(directions, np.float64)
    n, s = t.shape
    norm = np.sqrt((d * d).sum(-1))
    delta = np.concatenate((np.diff(t, axis=-1), np.full((n, 1), float(final_delta))), axis=-1)
    if mut == 'dirs_final_delta_dropped':
        delta[:, -1] = 0.0
    if mut == 'dirs_length_twice':
        delta = delta * norm[:, None]
    p = aux['bracket'] * (np.asarray(sigma, np.float64).reshape(n, s) * delta)
    with np.errstate(divide='ignore', invalid='ignore'):
        unit = d if mut == 'dirs_not_normalised' else np.where(norm[:, None] > 0, d / norm[:, None], 0.0)
    return unit * p.sum(-1)[:, None], p


def dirs_budget(fw, aux, directions, sigma, final_delta, d_sigma_bound):
    """(ref (N, 3), bound (N, 3)); d_sigma_bound: Y.backward_budget's bound on d_sigma for the same case (see the module docstring)"""
    ref, p = dirs_term_f64(fw, aux, directions, sigma, final_delta)
    d = np.asarray(directions, np.float64)
    n, s = p.shape
    norm = np.sqrt((d * d).sum(-1))
    length = np.abs(fw['length'])
    delta = np.concatenate((np.diff(fw['t'], axis=-1), np.full((n, 1), float(final_delta))), axis=-1)
    sd = np.abs(np.asarray(sigma, np.float64).reshape(n, s) * delta)
    with np.errstate(divide='ignore', invalid='ignore'):
        dq = np.where(length > 0, np.asarray(d_sigma_bound, np.float64) / length, 0.0)
        unit = np.where(norm[:, None] > 0, np.abs(d) / norm[:, None], 0.0)
    D = -(-s // 64) + 7
    dP = (sd * dq + 3.0 * U * np.abs(p)).sum(-1) + D * U * np.abs(p).sum(-1)
    return ref, (unit * dP[:, None] + 6.0 * U * np.abs(ref)) * Y.SECOND_ORDER
