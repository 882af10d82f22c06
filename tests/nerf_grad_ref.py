"""A float64 restatement, an exactness proof and per-element error budgets for the fused NeRF block's TRAINING backward (nerficg_amd/csrc/nerf_grad.hip:
k_nerf_dgrad, k_nerf_wgrad, k_nerf_wreduce; C ABI group 18, include/nerficg_hip.h; Python: nerficg_amd.nerf.fused_apply).  Plain module: no test functions.
The forward's restatement, the net containers, h16 / sat / gamma32 and the judges come from tests/nerf_mlp_ref.py (read its docstring first); used by
tests/test_nerf_grad_ref_cpu.py and tests/test_gpu_nerf_train.py.

The restatement (`head_gradients`, `data_gradient`, `weight_gradient`, `backward`)
---------------
S is the scale, a power of two.  `taps` are the saved fp16 operands of the forward (R.STAGES), `sigma` / `rgb` the f32 outputs the forward wrote.  A
gradient stage carries the name of the forward stage whose PRE-ACTIVATION it differentiates; BACKWARD_ORDER(net) = [rgb, C_1, F, sigma, H_L .. H_1].
    G[rgb]   = sat(h16(f32(f32(d_rgb S) f32(rgb f32(1 - rgb)))))        three f32 roundings (the product with S is exact), emulated exactly
    G[sigma] = sat(h16(f32(d_sigma S) [sigma > 0]))
    G[C_1]   = sat(h16(G[rgb] W16_rgb)) [C_1 > 0]
    G[F]     = sat(h16(G[C_1] W16_colour[:, :W]))                        no mask; the direction columns are not propagated
    G[H_L]   = sat(h16(G[F] W16_feature + G[sigma] w16_density)) [H_L > 0]   both consumers in ONE accumulator before the rounding
    G[H_l]   = sat(h16(G[H_l+1] W16_l[:, :W])) [H_l > 0]                 l = L-1 .. 1; the skip columns (behind the hidden ones) are not propagated
    dW_k     = (G[out_k]^T X_k) / S,  db_k = (sum_m G[out_k]) / S        X_k = the concatenated saved operands of linear k
W16 = sat(h16(W)).  Everything else is float64.

Exactness (`exact`)
-------------------
As in nerf_mlp_ref.exact: if every accumulator's sum of |addends| stays below 2^24 units (the unit a power of two dividing every addend) no partial sum in
any order rounds in f32, and if every dX is an fp16 number of magnitude <= 65504 the conversion does not round either: the device equals the restatement
bit for bit on every G stage, dW and db.  The exact family: R.exact_net (sparse +-1 weights), `exact_upstream` (signed powers of two on a few rows,
rgb in {1/4, 1/2, 3/4} so that rgb (1 - rgb) is 3/16 or 1/4 exactly -- the backward takes sigma and rgb as inputs, so a test may state them).
`shuffled_f32` re-adds one accumulator family in f32 in a random order: the module's own check that "exact" means what it says.

The budgets (u = 2^-24, gamma(k) = k u / (1 - k u))
-----------
One stage at a time, from the gradient stages the DEVICE produced (a chained budget would be vacuous, nerf_mlp_ref's docstring):
    G stage:  e = gamma(n_terms + 2) sum |W16| |G|; the device's value must lie between sat(h16(z - e)) and sat(h16(z + e)) where the mask keeps the
              element, and must be 0 where it does not.
    dW, db:   |device - restatement| <= gamma(M + 2) sum_m |G X| / S (+ one subnormal step 2^-149): the worst case of ANY summation order.
    heads:    the f32 sequence is emulated exactly: equality.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import nerf_mlp_ref as R
from tests.nerf_mlp_ref import gamma32, h16, sat, _conv_bound, judge, judge_interval  # noqa: F401  (re-exported for the tests)

MUTATIONS = ('drop_mask', 'mask_wrong_stage', 'mask_feature', 'drop_density', 'skip_offset', 'untransposed', 'sigmoid_rgb', 'bias_unscaled')


def BACKWARD_ORDER(net):
    assert net['n_color'] == 1
    return ['rgb', 'C_1', 'F', 'sigma'] + [f'H_{l}' for l in range(net['L'], 0, -1)]


def _w16(net, li):
    return sat(h16(net['lin'][li][0]))


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def head_gradients(sigma, rgb, d_sigma, d_rgb, S, mut=None, rounding=True, raw=False):
    """-> (G[rgb] (M, 3), G[sigma] (M, 1)) from f32 inputs, the device's f32 sequence step by step; raw: the f32 values in front of the fp16 conversion"""
    rd = _f32 if rounding else (lambda a: np.asarray(a, np.float64))     # the inputs are f32 numbers on the device
    sigma, rgb, d_sigma, d_rgb = rd(sigma).reshape(-1), rd(rgb).reshape(-1, 3), rd(d_sigma).reshape(-1), rd(d_rgb).reshape(-1, 3)
    with np.errstate(over='ignore', invalid='ignore'):
        slope = rgb if mut == 'sigmoid_rgb' else rd(rgb * rd(1.0 - rgb))
        g_rgb = rd(rd(d_rgb * S) * slope)
        g_sigma = np.where(sigma > 0.0, rd(d_sigma * S), 0.0)[:, None]
    if rounding and not raw:
        return sat(h16(g_rgb)), sat(h16(g_sigma))
    return g_rgb, g_sigma


def _consumers(net, name):
    """[(linear index, name of its gradient stage, first column, columns)] of the linears that read forward stage `name`; mask?"""
    L, W = net['L'], net['width']
    if name == 'C_1':
        return [(L + 3, 'rgb', 0, W // 2)], True
    if name == 'F':
        return [(L + 2, 'C_1', 0, W)], False
    kind, idx = name.split('_')
    idx = int(idx)
    assert kind == 'H'
    if idx == L:
        return [(L + 1, 'F', 0, W), (L, 'sigma', 0, W)], True
    return [(idx, f'H_{idx + 1}', 0, W)], True


def data_gradient(net, name, G, taps, mut=None, rounding=True):
    """Gradient stage `name` (C_1, F, H_l) from its consumers' stages in G -> dict(Z, out, mask, abs, n_terms)"""
    cons, masked = _consumers(net, name)
    W, n_pos = net['width'], R.n_enc(net['k_pos'], net['append'])
    Z, A, n_terms = 0.0, 0.0, 0
    for li, gname, c0, nc in cons:
        if mut == 'drop_density' and gname == 'sigma':
            continue
        w = _w16(net, li)
        if mut == 'skip_offset' and li in net['skips'] and name.startswith('H_'):
            c0 = n_pos
        w = w[:, c0:c0 + nc]
        if mut == 'untransposed' and w.shape[0] == w.shape[1] and name == 'H_2':
            w = w.T
        g = np.asarray(G[gname], np.float64)
        Z = Z + g @ w
        A = A + np.abs(g) @ np.abs(w)
        n_terms += g.shape[1]
    mask = np.ones_like(Z, bool)
    if masked or (mut == 'mask_feature' and name == 'F'):
        src = name
        if mut == 'mask_wrong_stage' and name.startswith('H_') and int(name[2:]) >= 2:
            src = f'H_{int(name[2:]) - 1}'
        mask = np.asarray(taps[src], np.float64) > 0.0
        if mut == 'drop_mask' and name == 'H_2':
            mask = np.ones_like(Z, bool)
    out = np.where(mask, sat(h16(Z)) if rounding else Z, 0.0)
    return dict(Z=Z, out=out, mask=mask, abs=A, n_terms=n_terms)


def linear_operand(net, li, taps):
    """the concatenated saved operands of linear li and the name of its gradient stage"""
    L = net['L']
    out_name = [f'H_{l + 1}' for l in range(L)] + ['sigma', 'F', 'C_1', 'rgb']
    names = R.stage_operands(net, out_name[li])
    return np.concatenate([np.asarray(taps[n], np.float64) for n in names], axis=1), out_name[li]


def weight_gradient(net, li, G, taps, S, mut=None):
    """-> dict(dW, db, absW, absb): the sums over the rows divided by S, and the sums of |addends| / S"""
    X, gname = linear_operand(net, li, taps)
    g = np.asarray(G[gname], np.float64)
    return dict(dW=g.T @ X / S, db=g.sum(axis=0) / (1.0 if mut == 'bias_unscaled' else S), absW=np.abs(g).T @ np.abs(X) / S, absb=np.abs(g).sum(axis=0) / S)


def backward(net, taps, sigma, rgb, d_sigma, d_rgb, S, mut=None, rounding=True):
    """-> dict(G={stage: (M, width)}, dW=[...], db=[...]) in float64 with the contract's roundings (rounding=False: no fp16 rounding of the gradients and no
    f32 rounding of the heads -- the plain chain rule through the fp16 weights and saved operands, for the comparison with autograd).  mut: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS
    G = {}
    G['rgb'], G['sigma'] = head_gradients(sigma, rgb, d_sigma, d_rgb, S, mut, rounding)
    for name in BACKWARD_ORDER(net):
        if name not in G:
            G[name] = data_gradient(net, name, G, taps, mut, rounding)['out']
    wg = [weight_gradient(net, li, G, taps, S, mut) for li in range(len(net['lin']))]
    return dict(G=G, dW=[w['dW'] for w in wg], db=[w['db'] for w in wg])


# ------------------------------------------------------------------------------------------------ exactness
def exact(net, taps, sigma, rgb, d_sigma, d_rgb, S, bw=None):
    """(ok, worst accumulator ratio): every head gradient an fp16 number before its conversion, every dX an fp16 number, every accumulator (dX, dW, db)
    below 2^24 units -- then the device's bits are the restatement's whatever its order of summation."""
    bw = backward(net, taps, sigma, rgb, d_sigma, d_rgb, S) if bw is None else bw
    raw = head_gradients(sigma, rgb, d_sigma, d_rgb, S, rounding=False)
    ok = all(bool(np.all(h16(r) == r) and np.all(np.abs(r) <= R.H16_MAX)) for r in raw)
    ratios = []
    for name in BACKWARD_ORDER(net):
        if name in ('rgb', 'sigma'):
            continue
        st = data_gradient(net, name, bw['G'], taps)
        ok = ok and bool(np.all(h16(st['Z']) == st['Z'])) and bool(np.all(np.abs(st['Z']) <= R.H16_MAX))
        for li, gname, c0, nc in _consumers(net, name)[0]:
            ratios.append(R._acc_ratio(bw['G'][gname], _w16(net, li)[:, c0:c0 + nc], np.zeros(nc)))
    for li in range(len(net['lin'])):
        X, gname = linear_operand(net, li, taps)
        g = bw['G'][gname]
        ratios.append(R._acc_ratio(g.T, X, np.zeros(X.shape[1])))
        ratios.append(R._acc_ratio(g.T, np.ones((g.shape[0], 1)), np.zeros(1)))
    return bool(ok and max(ratios) < 1.0), max(ratios)


def shuffled_f32(A, B, rng):
    """A @ B with every product added in f32, one by one, in a random order of the inner index (any device order is one of these)"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in rng.permutation(A.shape[1]):
        acc = (acc + A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)
    return acc.astype(np.float64)


@functools.lru_cache(maxsize=None)
def exact_net(width, n_layers=8, skips=(5,), k_pos=0, k_dir=0, seed=0):
    """The recipe of R.exact_net with ONE colour layer (what the training path supports) and a free shape: sparse +-1 weights, small dyadics in the
    heads, small integer biases.  K = 0 with append_input: the encoding is the identity (inputs: R.exact_inputs(m, 'identity')); K > 0: inputs 0."""
    rng = np.random.default_rng([seed, width, n_layers, k_pos, 31])
    n_pos, n_dir, half = R.n_enc(k_pos, True), R.n_enc(k_dir, True), width // 2
    ib = lambda n, hi=2: rng.integers(0, hi + 1, size=n).astype(np.float64)
    lin = [(R._sparse(rng, width, n_pos, 2), ib(width))]
    for l in range(1, n_layers):
        W = R._sparse(rng, width, width, 2)
        if l in skips:
            W = np.concatenate([W, R._sparse(rng, width, n_pos, 1)], axis=1)
        lin.append((W, ib(width, 1)))
    lin.append((R._sparse(rng, 1, width, 8, (-0.25, 0.25, 0.5)), ib(1)))
    lin.append((R._sparse(rng, width, width, 2), ib(width, 3) - 1.0))
    lin.append((np.concatenate([R._sparse(rng, half, width, 2), R._sparse(rng, half, n_dir, 1)], axis=1), ib(half, 1)))
    lin.append((R._sparse(rng, 3, half, 6, (-0.0625, 0.0625, 0.125)), ib(3, 1) - 0.5))
    return R.make_net(lin, n_layers, 1, k_pos, k_dir, True, skips)


def exact_upstream(m, seed=0, rows=48):
    """(d_sigma (M,), d_rgb (M, 3), sigma (M,), rgb (M, 3)) f32: signed powers of two on at most `rows` rows (the first and the last among them) and
    zeros elsewhere, so that a weight gradient over thousands of rows stays exact; sigma in {0, 1}, rgb in {1/4, 1/2, 3/4}."""
    rng = np.random.default_rng([seed, m, 23])
    d_sigma, d_rgb = np.zeros(m, np.float32), np.zeros((m, 3), np.float32)
    pick = np.unique(np.concatenate([[0, m - 1], rng.choice(m, size=min(rows, m), replace=False)]))
    d_sigma[pick] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=pick.size)
    d_rgb[pick] = rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0, 4.0], size=(pick.size, 3))
    sigma = rng.choice([0.0, 1.0], size=m, p=[0.25, 0.75]).astype(np.float32)
    rgb = rng.choice([0.25, 0.5, 0.75], size=(m, 3)).astype(np.float32)
    return d_sigma, d_rgb, sigma, rgb


def centre_density(net, positions, directions):
    """The net with its density bias moved (to an f32 number) so that about half of these rows have sigma > 0: a freshly initialised block is negative
    on most of space, and a density head that never opens tests nothing."""
    z = R.layer(net, 'sigma', R.forward(net, positions, directions))['Z'][:, 0]
    lin = list(net['lin'])
    w, b = lin[net['L']]
    lin[net['L']] = (w, np.asarray(b - np.median(z), np.float32).astype(np.float64))
    return R.make_net(lin, net['L'], net['n_color'], net['k_pos'], net['k_dir'], net['append'], net['skips'])


def random_upstream(m, seed=0, scale=1.0):
    """upstream gradients of the size an MSE loss behind the compositing gives them: normal, about 1e-3 `scale`"""
    rng = np.random.default_rng([seed, m, 29])
    return (rng.normal(size=m) * 1e-3 * scale).astype(np.float32), (rng.normal(size=(m, 3)) * 1e-3 * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ budgets
def stage_budget(net, name, G, taps):
    """(ref, bound) of gradient stage `name` from the gradient stages in G (the device's own): bound 0 where the mask drops the element"""
    st = data_gradient(net, name, G, taps)
    e = gamma32(st['n_terms'] + 2) * st['abs']
    return st['out'], np.where(st['mask'], _conv_bound(st['Z'], e, sat(h16(st['Z'])), act=False), 0.0)


def weight_budget(net, li, G, taps, S):
    """((dW, bound), (db, bound)) of linear li from the gradient stage in G (the device's own) and the saved operands"""
    wg = weight_gradient(net, li, G, taps, S)
    m = np.asarray(G[linear_operand(net, li, taps)[1]]).shape[0]
    tiny = 2.0 ** -149
    return (wg['dW'], gamma32(m + 2) * wg['absW'] + tiny), (wg['db'], gamma32(m + 2) * wg['absb'] + tiny)


def chained_check(net, taps, sigma, rgb, d_sigma, d_rgb, S, got):
    """Every stage of `got` (dict(G, dW, db): a device's, or a mutant restatement's) against the restatement applied to got's OWN previous stages.
    -> {name: (elements over their bound, worst error / bound)}"""
    res = {}
    g_rgb, g_sigma = head_gradients(sigma, rgb, d_sigma, d_rgb, S)
    for name, ref in (('rgb', g_rgb), ('sigma', g_sigma)):
        res[f'G[{name}]'] = (int(np.count_nonzero(np.asarray(got['G'][name], np.float64).reshape(ref.shape) != ref)), 0.0)
    for name in BACKWARD_ORDER(net):
        if name in ('rgb', 'sigma'):
            continue
        ref, bound = stage_budget(net, name, got['G'], taps)
        ratio, over = judge(np.asarray(got['G'][name], np.float64), ref, bound)
        res[f'G[{name}]'] = (over, ratio)
    for li in range(len(net['lin'])):
        (dw, bw_), (db, bb) = weight_budget(net, li, got['G'], taps, S)
        ratio, over = judge(np.asarray(got['dW'][li], np.float64).reshape(dw.shape), dw, bw_)
        res[f'dW[{li}]'] = (over, ratio)
        ratio, over = judge(np.asarray(got['db'][li], np.float64).reshape(db.shape), db, bb)
        res[f'db[{li}]'] = (over, ratio)
    return res


def exact_check(bw, got):
    """Names of the stages of `got` that differ from the restatement `bw` of an exact case, bit for bit"""
    bad = [f'G[{n}]' for n in bw['G'] if not np.array_equal(np.asarray(got['G'][n], np.float64).reshape(bw['G'][n].shape), bw['G'][n])]
    for key in ('dW', 'db'):
        bad += [f'{key}[{li}]' for li, ref in enumerate(bw[key]) if not np.array_equal(np.asarray(got[key][li], np.float64).reshape(ref.shape), ref)]
    return bad
