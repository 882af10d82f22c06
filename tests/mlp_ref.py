"""A float64 restatement, an exactness proof and a per-element error budget for the fully fused MLP (nerficg_amd/csrc/ngp_net.hip: k_nwie_fwd, k_nwie_bwd;
C ABI nrc_nwie_forward / nrc_nwie_backward, include/nerficg_hip.h).  Plain module: no test functions.  Used by tests/test_mlp_ref_cpu.py and
tests/test_gpu_mlp_grad.py; tests/frame_stage_ref.py takes the forward half (`forward_budget`) for the image frame's two networks.

The restatement
---------------
Weights [W0 (64,32) | hidden (64,64) x (n_hidden-1) | Wout (16,64)], rows of Wout at and behind n_out_rows read as zero.  X (M,32) are the encoded inputs;
for encoding 1: [fp16(SH4(2 d01 - 1)) (16) | identity (16)], the SH columns taken from oracle.sh4_encode (`encode`).  fp16(.) is round-to-nearest-even.
    forward    Z_l = H_{l-1} W_l^T (H_{-1} = X),  H_l = max(fp16(Z_l), +0),  Z_out = H_last Wout^T,  out = fp16(act(Z_out))
    backward   dZ_out = fp16(g [y (1 - y)] loss_scale)   (columns < n_out_rows; y = the `out` handed to the call, read for the sigmoid only)
               dH = dZ W   ;   dZ_l = fp16(dH) where H_l > 0, else 0
               dW_l = old_l + dZ_l^T H_{l-1} / loss_scale   ;   d_in = dZ_0 W_0 / loss_scale
Everything else is float64.  A unit is alive iff H > 0: a pre-activation that rounds to fp16 -0 or +0 is dead.

Exactness (`exact`)
-------------------
If (a) every value the kernels convert to fp16 (each Z_l, Z_out, dZ_out, each dH) is an fp16 number already, and (b) for every f32 accumulator (each Z,
dH, d_in, every dW element over all M samples plus the caller's old value) with `unit` a power of two that divides every addend the sum of |addends| is
below 2^24 unit, then every partial sum of the addends, in any order and any grouping, is a multiple of `unit` below 2^24 unit in magnitude -- an f32
number -- so no addition ever rounds: MFMA chains, the four-wave LDS reduction and the memory atomics give the mathematical sum, the conversions of (a)
do not round, and products of two fp16 numbers are exact in f32.  loss_scale must be a power of two (its reciprocal and both scalings are then exact).
The device result equals the restatement BIT FOR BIT.  `unit` is taken conservatively as (smallest low bit of a non-zero entry in the one operand's row)
x (the same of the other operand's column), which divides every product; a smaller unit only makes (b) stricter.  Float64 sums of such addends are exact as
well (2^24 < 2^53), whatever order BLAS takes.

The budget (`budget`; u = 2^-24, gamma(k) = k u / (1 - k u))
----------
For inputs that are not exact every element gets an absolute bound on |device - restatement|, carried layer by layer as E.
  f32 sum of K products in any order, operands off by E:   e_Z = |W| E_prev + gamma(K + 1) |W| (|H_prev| + E_prev)
      (products of fp16 numbers are exact; K - 1 additions at most on any addend's path, + 2 of slack for the accumulator's start and a final scaling)
  conversion to fp16: rounding is monotone, so the device value lies in [fp16(Z - e_Z), fp16(Z + e_Z)] (after max(., +0) for an activation): the bound is
      the larger distance of those two from the restated value -- ZERO unless an fp16 rounding boundary (the one between 0 and the smallest subnormal
      included) lies inside the interval, one fp16 ulp (or more, if e_Z spans more) when it does.
  ReLU mask: if max(fp16(Z - e_Z), 0) == 0 < max(fp16(Z + e_Z), 0) the device may see the unit either way: the candidates for its dZ are 0, fp16(dH - e)
      and fp16(dH + e), i.e. the whole |dH| enters the bound.
  dZ_out: g [y (1 - y)] loss_scale is three f32 products (1 - y is exact for an fp16 y): e = gamma(3) |v| in front of the conversion; without the
      sigmoid g loss_scale is exact.
  weight gradient, element (o, c), n = number of samples whose addend CAN be non-zero ((|dZ| + E_dZ)(|P| + E_P) > 0):
      [ |dZ|^T E_P + E_dZ^T (|P| + E_P)  +  gamma(n + 2) (|dZ| + E_dZ)^T (|P| + E_P) ] / loss_scale  +  gamma(n + 2) |old|
      -- the propagated operand bounds; n addends summed in some tree (registers, LDS, at most one atomic per workgroup: depth <= n - 1), one scaling by
      1 / loss_scale per partial (+ 1), and the old value as one more addend at the bottom of at most min(n, workgroups) atomics (+ 1, and its own share).
      n == 0: the element must come back with the bits it went in with (budget 0).
  d_in: the e_Z formula over the 64 units (K = 64, its + 1 covers the scaling), divided by loss_scale.
  sigmoid output: faithful rounding -- the device value must lie in [fp16_down(s(o - e_o)), fp16_up(s(o + e_o))], s the float64 sigmoid; f32 expf and
      the division are below 2^-21 relative, far under half an fp16 ulp (2^-12), so the round-to-nearest of the f32 value is one of the two neighbours.
  SH inputs (GPU only): sh4_eval is at most 8 f32 roundings of intermediates below 4 in magnitude: e = 4 gamma(8) around the float64 value, through the
      conversion rule above (`sh_input_bound`); the CPU oracle shares oracle.sh4_encode with the restatement (E = 0).
The float64 restatement's own rounding (2^-53 relative to the same sums) is 2^-29 of any gamma term and is ignored.  No measured constant, no tensor
maximum and no excluded element enter.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle

U32 = 2.0 ** -24
W0_N, WH_N, WO_N = 64 * 32, 64 * 64, 16 * 64


def gamma32(k):
    k = np.asarray(k, np.float64)
    return k * U32 / (1.0 - k * U32)


def h16(a):
    with np.errstate(over='ignore'):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def h16_down(a):
    a = np.asarray(a, np.float64)
    r = a.astype(np.float16)
    return np.where(r.astype(np.float64) > a, np.nextafter(r, np.float16(-np.inf)), r).astype(np.float64)


def h16_up(a):
    return -h16_down(-np.asarray(a, np.float64))


def relu(h):
    return np.maximum(h, 0.0) + 0.0   # (+ 0.0: a -0.0 that maximum may hand back becomes +0.0)


def n_weights(n_hidden):
    return W0_N + (n_hidden - 1) * WH_N + WO_N


def layers(W, n_hidden, n_out_rows=16):
    W = np.asarray(W, np.float64).reshape(-1)
    assert W.size == n_weights(n_hidden)
    Ws, off = [W[:W0_N].reshape(64, 32)], W0_N
    for _ in range(n_hidden - 1):
        Ws.append(W[off:off + WH_N].reshape(64, 64))
        off += WH_N
    Wo = W[off:].reshape(16, 64).copy()
    Wo[n_out_rows:] = 0.0
    return Ws, Wo


def sh4_f64(d01):
    """degree-4 spherical harmonics of 2 d01 - 1 in float64 (the formulas of oracle/tcnn_oracle.c and ngp_net.h)"""
    d = np.asarray(d01, np.float64) * 2.0 - 1.0
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    o = [0.28209479177387814 + 0 * x, -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x, 1.0925484305920792 * xy,
         -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
         0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
         0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
         1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)]
    return np.stack(o, 1)


def encode(x16):
    """input rows (M, >= 19) fp16 [d01 (3) | identity (16)] -> X (M,32) float64"""
    x = np.asarray(x16, np.float16)
    return np.concatenate([oracle.sh4_encode(x[:, :3].astype(np.float32)).astype(np.float64), x[:, 3:19].astype(np.float64)], 1)


def sh_input_bound(x16, X):
    """E_X (M,32) for a device that evaluates the SH columns itself (f32)"""
    E = np.zeros_like(X)
    E[:, :16] = _conv_bound(sh4_f64(np.asarray(x16, np.float16)[:, :3]), 4.0 * gamma32(8), X[:, :16])
    return E


def _pad16(a, m):
    out = np.zeros((m, 16))
    if a is not None:
        a = np.asarray(a, np.float64)
        out[:, :a.shape[1]] = a
    return out


def forward(X, W, n_hidden, out_act, n_out_rows=16, rounding=True, hidden=None):
    """hidden: (Z, H) of an earlier call with the same X, W and n_hidden (they do not depend on the output layer's shape or activation)"""
    Ws, Wo = layers(W, n_hidden, n_out_rows)
    rd = h16 if rounding else (lambda a: a)
    H, Z = [np.asarray(X, np.float64)], []
    if hidden is not None:
        Z, H = list(hidden[0]), H + list(hidden[1])
    else:
        for Wl in Ws:
            Z.append(H[-1] @ Wl.T)
            H.append(relu(rd(Z[-1])))
    zo = H[-1] @ Wo.T
    with np.errstate(over='ignore'):
        out = rd(1.0 / (1.0 + np.exp(-zo)) if out_act else zo)
    return dict(X=H[0], Z=Z, H=H[1:], Zout=zo, out=out)


MUTATIONS = ('drop_last_row', 'swap_grad_rows', 'open_dead_relu', 'skip_wout_row', 'transpose_dw1_block', 'forget_old', 'loss_scale_one_way')


def backward(fw, W, g, y, loss_scale, n_hidden, out_act, n_out_rows=16, old=None, rounding=True, mut=None, detail=False):
    """g, y: (M, k <= 16) upstream gradient and the `out` the call is given.  Returns (dW flat incl. old, d_in (M,32)) float64.
    mut: one of MUTATIONS -- a deliberately wrong restatement (tests/test_mlp_ref_cpu.py shows that the checks notice each)."""
    assert mut is None or mut in MUTATIONS
    Ws, Wo = layers(W, n_hidden, n_out_rows)
    rd = h16 if rounding else (lambda a: a)
    m, ls = fw['X'].shape[0], float(loss_scale)
    g, y = _pad16(g, m), _pad16(y, m)
    v = g * (y * (1.0 - y) if out_act else 1.0) * ls
    dZo = rd(v)
    dZo[:, n_out_rows:] = 0.0
    if mut == 'drop_last_row':
        dZo[m - 1] = 0.0
    if mut == 'swap_grad_rows':
        j = int(np.argmax(np.any(dZo != dZo[0], axis=1)))
        dZo[[0, j]] = dZo[[j, 0]]
    if mut == 'skip_wout_row':
        dZo[:, n_out_rows - 1] = 0.0
    rows = np.flatnonzero(np.any(dZo != 0, axis=1))   # every backward quantity of the other rows is zero
    dZo = dZo[rows]
    dWs = [None] * n_hidden
    dWo = dZo.T @ fw['H'][-1][rows]
    dH = dZo @ Wo
    pre = dict(v=v, rows=rows, dH=[dH])   # dH: the live rows only
    for l in range(n_hidden - 1, -1, -1):
        alive = fw['H'][l][rows] > 0
        if mut == 'open_dead_relu' and l == n_hidden - 1:
            k = np.unravel_index(np.argmax(np.where(alive, 0.0, np.abs(rd(dH)))), dH.shape)
            alive[k] = True
        dZ = np.where(alive, rd(dH), 0.0)
        dWs[l] = dZ.T @ (fw['H'][l - 1] if l > 0 else fw['X'])[rows]
        dH = dZ @ Ws[l]
        pre['dH'].append(dH)
    d_in = np.zeros((m, 32))
    d_in[rows] = dH
    if mut == 'transpose_dw1_block':
        dWs[1][:32, :32] = dWs[1][:32, :32].T.copy()
    back = 1.0 if mut == 'loss_scale_one_way' else ls
    dW = np.concatenate([a.reshape(-1) for a in dWs] + [dWo.reshape(-1)]) / back
    if old is not None and mut != 'forget_old':
        dW = dW + np.asarray(old, np.float64).reshape(-1)
    return (dW, d_in / back, pre) if detail else (dW, d_in / back)


# ------------------------------------------------------------------------------------------------ exactness
def _bits(a):
    """entries as integers in units of 2^-40 (they must be multiples of 2^-40 below 2^22)"""
    s = np.abs(np.asarray(a, np.float64)) * 2.0 ** 40
    n = s.astype(np.int64)
    assert np.all(n == s), 'value finer than 2^-40'
    return n


def _low(n):
    """largest power of two dividing the integers n x 2^-40 (inf for 0)"""
    return np.where(n == 0, np.inf, (n & -n).astype(np.float64) * 2.0 ** -40)


def _acc_ratio(A, B, extra=None):
    """accumulators (A @ B)[i, j] (+ extra[i, j]): sum |addends| / (2^24 unit), unit = minlow(A[i, :]) minlow(B[:, j]) (and the low bit of extra);
    the smallest low bit of a row is the low bit of the OR of its entries"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    unit = np.outer(_low(np.bitwise_or.reduce(_bits(A), axis=1)), _low(np.bitwise_or.reduce(_bits(B), axis=0)))
    s = np.abs(A) @ np.abs(B)
    if extra is not None:
        unit = np.minimum(unit, _low(_bits(extra)))
        s = s + np.abs(extra)
    return float(np.max(np.where(s > 0, s / (2.0 ** 24 * np.where(np.isfinite(unit), unit, 1.0)), 0.0), initial=0.0))


def _hidden_exact(fw, Ws):
    """the forward's hidden layers: (pre-activations are fp16 numbers, their largest magnitude, accumulator ratios)"""
    Hs = [fw['X']] + fw['H']
    return (all(bool(np.all(h16(z) == z)) for z in fw['Z']), max(float(np.abs(z).max(initial=0.0)) for z in fw['Z']),
            [_acc_ratio(Hs[l], Wl.T) for l, Wl in enumerate(Ws)])


def exact(X, W, g, y, loss_scale, n_hidden, out_act, n_out_rows=16, old=None, _fw=None, _pre=None, _hid=None):
    """(ok, fp16_max, acc_max): both conditions of the module docstring; fp16_max = largest magnitude converted to fp16 (the integers up to 2048 are
    fp16 numbers), acc_max = largest sum |addends| / (2^24 unit) over every f32 accumulator (must stay below 1)."""
    ls = float(loss_scale)
    ok = np.log2(ls) == np.round(np.log2(ls))
    Ws, Wo = layers(W, n_hidden, n_out_rows)
    fw = forward(X, W, n_hidden, 0, n_out_rows) if _fw is None else _fw   # (the output activation plays no part below)
    pre = backward(fw, W, g, y, ls, n_hidden, out_act, n_out_rows, old, detail=True)[2] if _pre is None else _pre
    ok_h, fp16_max, acc = _hidden_exact(fw, Ws) if _hid is None else _hid
    ok, acc, Hs = ok and ok_h, list(acc), [fw['X']] + fw['H']
    for a in ([fw['Zout']] if not out_act else []) + [pre['v']] + pre['dH'][:-1]:
        ok = ok and bool(np.all(h16(a) == a))
        fp16_max = max(fp16_max, float(np.abs(a).max(initial=0.0)))
    acc.append(_acc_ratio(Hs[-1], Wo.T))
    rows = pre['rows']
    dZo = h16(pre['v'][rows])
    dZo[:, n_out_rows:] = 0.0
    oldl = (np.zeros(n_weights(n_hidden)) if old is None else np.asarray(old, np.float64).reshape(-1)) * ls
    offs = np.cumsum([0] + [w.size for w in Ws])
    acc.append(_acc_ratio(dZo.T, Hs[-1][rows], oldl[offs[-1]:].reshape(16, 64)))
    acc.append(_acc_ratio(dZo, Wo))
    for i, l in enumerate(range(n_hidden - 1, -1, -1)):
        dZ = np.where(fw['H'][l][rows] > 0, h16(pre['dH'][i]), 0.0)
        acc.append(_acc_ratio(dZ.T, Hs[l][rows], oldl[offs[l]:offs[l + 1]].reshape(Ws[l].shape)))
        acc.append(_acc_ratio(dZ, Ws[l]))
    acc_max = max(acc)
    return bool(ok and acc_max < 1.0), fp16_max, acc_max


# ------------------------------------------------------------------------------------------------ budget
def _conv_bound(z, e, ref, act=False):
    lo, hi = h16(z - e), h16(z + e)
    if act:
        lo, hi = relu(lo), relu(hi)
    return np.maximum(np.abs(lo - ref), np.abs(hi - ref))


def _sum_bound(E, P, Wt, k):
    """|device - restated| of P @ Wt with operand bound E on P, k addends"""
    aw = np.abs(Wt)
    return E @ aw + gamma32(k + 1) * ((np.abs(P) + E) @ aw)


def _dw_bound(dZ, EdZ, P, EP, old, ls):
    a, b = np.abs(dZ) + EdZ, np.abs(P) + EP
    n = (a > 0).astype(np.float64).T @ (b > 0).astype(np.float64)
    cross = np.abs(dZ).T @ EP + EdZ.T @ b
    return (cross + gamma32(n + 2) * (a.T @ b)) / ls + gamma32(n + 2) * np.abs(old)


def forward_budget(X, W, n_hidden, out_act, n_out_rows=16, E_X=None):
    """The forward half of `budget`: the restated forward pass and, layer by layer, the bound E on |device - restated| of every activation, from the bound
    E_X (M,32) on the inputs (None: exact inputs).  Returns dict(fw=..., Hs=[X, H_0, ...], Es=[E_X, E_0, ...], flips=[units whose ReLU mask the device may
    see either way, per layer], e_out=bound on Z_out in front of the conversion, out=(lo, hi) fp16 interval per output, out_ref=the restated output)."""
    Ws, Wo = layers(W, n_hidden, n_out_rows)
    fw = forward(X, W, n_hidden, out_act, n_out_rows)
    E = np.zeros_like(fw['X']) if E_X is None else np.asarray(E_X, np.float64)
    Hs, Es, flips = [fw['X']] + fw['H'], [E], []
    for l, Wl in enumerate(Ws):
        eZ = _sum_bound(Es[-1], Hs[l], Wl.T, Wl.shape[1])
        flips.append((relu(h16(fw['Z'][l] - eZ)) == 0) & (relu(h16(fw['Z'][l] + eZ)) > 0))
        Es.append(_conv_bound(fw['Z'][l], eZ, fw['H'][l], act=True))
    eo = _sum_bound(Es[-1], Hs[-1], Wo.T, 64)
    if out_act:
        with np.errstate(over='ignore'):
            out_iv = (h16_down(1.0 / (1.0 + np.exp(-(fw['Zout'] - eo)))), h16_up(1.0 / (1.0 + np.exp(-(fw['Zout'] + eo)))))
    else:
        out_iv = (h16(fw['Zout'] - eo), h16(fw['Zout'] + eo))
    return dict(fw=fw, Hs=Hs, Es=Es, flips=flips, e_out=eo, out=out_iv, out_ref=fw['out'])


def budget(X, W, g, y, loss_scale, n_hidden, out_act, n_out_rows=16, old=None, E_X=None):
    """Per-element bounds of the module docstring.  y: the `out` the backward call is GIVEN (an input of the call: no bound of its own).
    Returns dict(out=(lo, hi) fp16 interval per output, dW=flat bound, d_in=(M,32) bound, fw=..., dW_ref=..., d_in_ref=...)."""
    ls = float(loss_scale)
    Ws, Wo = layers(W, n_hidden, n_out_rows)
    fb = forward_budget(X, W, n_hidden, out_act, n_out_rows, E_X)
    fw, Hs, Es, flips, out_iv = fb['fw'], fb['Hs'], fb['Es'], fb['flips'], fb['out']
    # backward
    oldf = np.zeros(n_weights(n_hidden)) if old is None else np.asarray(old, np.float64).reshape(-1)
    offs = np.cumsum([0] + [w.size for w in Ws])
    dW_ref, d_in_ref, pre = backward(fw, W, g, y, ls, n_hidden, out_act, n_out_rows, old, detail=True)
    rows = pre['rows']   # a row whose dZ_out is zero has e = 0 there (v = 0) and adds nothing to any bound: its d_in must be exactly 0
    v = pre['v'][rows]
    dZo = h16(v)
    EdZ = _conv_bound(v, gamma32(3) * np.abs(v) if out_act else 0.0, dZo)
    dZo[:, n_out_rows:] = 0.0
    EdZ[:, n_out_rows:] = 0.0
    bW = [None] * n_hidden
    bWo = _dw_bound(dZo, EdZ, Hs[-1][rows], Es[-1][rows], oldf[offs[-1]:].reshape(16, 64), ls)
    e = _sum_bound(EdZ, dZo, Wo, 16)
    for i, l in enumerate(range(n_hidden - 1, -1, -1)):
        dH = pre['dH'][i]
        alive = fw['H'][l][rows] > 0
        dZ = np.where(alive, h16(dH), 0.0)
        lo, hi = h16(dH - e), h16(dH + e)
        near = np.maximum(np.abs(lo - dZ), np.abs(hi - dZ))
        EdZ = np.where(flips[l][rows], np.maximum(near, np.abs(dZ)), np.where(alive, near, 0.0))
        bW[l] = _dw_bound(dZ, EdZ, Hs[l][rows], Es[l][rows], oldf[offs[l]:offs[l + 1]].reshape(Ws[l].shape), ls)
        e = _sum_bound(EdZ, dZ, Ws[l], 64)
    b_in = np.zeros_like(fw['X'])
    b_in[rows] = e / ls
    return dict(out=out_iv, out_ref=fw['out'], dW=np.concatenate([b.reshape(-1) for b in bW] + [bWo.reshape(-1)]), d_in=b_in, dW_ref=dW_ref,
                d_in_ref=d_in_ref, fw=fw)


def judge(got, ref, bound):
    """(worst error / bound over the elements with a bound, number of elements over their bound); a zero bound demands equality"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    over = int(np.count_nonzero(~(err <= bound)))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.max(np.where(bound > 0, err / bound, 0.0), initial=0.0))
    return ratio, over


def judge_interval(got, iv):
    got = np.asarray(got, np.float64)
    return int(np.count_nonzero(~((got >= iv[0]) & (got <= iv[1]))))


# ------------------------------------------------------------------------------------------------ cases
def _ternary(rng, shape, density):
    return rng.choice([-1.0, 1.0], size=shape) * (rng.random(shape) < density)


def live_rows(m, rng):
    """rows with a non-zero upstream gradient: all of a small batch; of a large one the first 64, the last 64 and ~0.5 % at random"""
    live = np.ones(m, bool)
    if m > 256:
        live = rng.random(m) < 0.005
        live[:64] = True
        live[-64:] = True
    return live


@functools.lru_cache(maxsize=None)
def _exact_net(m, n_hidden, grid, seed):
    rng = np.random.default_rng([seed, m, n_hidden, int(grid)])
    W0 = np.zeros((64, 32))
    W0[:, 16:] = _ternary(rng, (64, 16), 0.25)
    if grid:
        W0[:, :16] = _ternary(rng, (64, 16), 0.25)
    Wl = [W0] + [_ternary(rng, (64, 64), 0.12) for _ in range(n_hidden - 1)] + [_ternary(rng, (16, 64), 0.5)]
    W = np.concatenate([w.reshape(-1) for w in Wl])
    if grid:
        x16, X = None, np.repeat(rng.integers(0, 4, size=(1, 32)).astype(np.float64), m, axis=0)
    else:
        x16 = np.concatenate([rng.choice([0.0, 0.5, 1.0], size=(m, 3)), rng.integers(0, 4, size=(m, 16)).astype(np.float64)], 1).astype(np.float16)
        X = encode(x16)
    fw = forward(X, W, n_hidden, 0)
    return dict(W=W, x16=x16, X=X, hidden=(fw['Z'], fw['H']), hid=_hidden_exact(fw, layers(W, n_hidden)[0]))


@functools.lru_cache(maxsize=None)
def exact_case(m, n_hidden, out_act, loss_scale=128.0, n_out_rows=16, with_old=False, seed=0, g_cols=16, grid=False):
    """A provably exact input set (module docstring).  Ternary weights (SH columns of W0 zero), identity inputs 0..3, d01 in {0, 0.5, 1}^3, gradients
    integers in [-2, 2] / loss_scale on the live rows and the first g_cols columns (sigmoid: multiples of 16 / loss_scale in [-1, 1] x 16, out in
    {0.25, 0.5, 0.75}).  grid: no x16; all 32 columns of W0 are ternary and X is ONE row of integers 0..3 for every sample (the features of a hash grid
    with a constant table per level, at any position).  Returns a dict of read-only arrays with the restatement's results and the exactness margins."""
    net = _exact_net(m, n_hidden, grid, seed)   # weights and inputs: one set (and one forward through the hidden layers) per (m, n_hidden)
    W, x16, X = net['W'], net['x16'], net['X']
    rng = np.random.default_rng([seed, m, n_hidden, out_act, n_out_rows, int(grid), 1])
    live = live_rows(m, rng)
    live = live[:, None] & (np.arange(16) < g_cols)[None, :]
    if out_act:
        k = rng.integers(-1, 2, size=(m, 16)) * live
        g = (16.0 * k / loss_scale)
        y = rng.choice([0.25, 0.5, 0.75], size=(m, 16))
    else:
        k = rng.integers(-2, 3, size=(m, 16)) * live
        g, y = k / loss_scale, None
    old = None
    if with_old:
        old = rng.integers(-3, 4, size=n_weights(n_hidden)).astype(np.float32)   # (old x loss_scale shares the accumulator's 24 bits)
    return finish_case(dict(m=m, n_hidden=n_hidden, out_act=out_act, loss_scale=float(loss_scale), n_out_rows=n_out_rows, W=W, x16=x16, X=X,
                            g=g.astype(np.float16), y=None if y is None else y.astype(np.float16), old=old, _hidden=net['hidden'], _hid=net['hid']))


def finish_case(c, need_exact=True):
    """adds X, the restatement's fw / dW / d_in and the margins; asserts exactness; freezes the arrays"""
    assert np.all(c['g'].astype(np.float64) * c['loss_scale'] == np.round(c['g'].astype(np.float64) * c['loss_scale']))
    if c.get('X') is None:
        c['X'] = encode(c['x16'])
    c['fw'] = forward(c['X'], c['W'], c['n_hidden'], c['out_act'], c['n_out_rows'], hidden=c.pop('_hidden', None))
    c['dW'], c['d_in'], pre = backward(c['fw'], c['W'], c['g'], c['y'], c['loss_scale'], c['n_hidden'], c['out_act'], c['n_out_rows'], c['old'], detail=True)
    c['exact'], c['fp16_max'], c['acc_max'] = ok, _, _ = exact(c['X'], c['W'], c['g'], c['y'], c['loss_scale'], c['n_hidden'], c['out_act'], c['n_out_rows'],
                                                                 c['old'], _fw=c['fw'], _pre=pre, _hid=c.pop('_hid', None))
    assert ok or not need_exact, f"case is not provably exact: largest fp16-converted magnitude {c['fp16_max']}, accumulator margin {c['acc_max']}"
    for a in [c[k] for k in ('W', 'x16', 'g', 'y', 'old', 'X', 'dW', 'd_in')] + c['fw']['Z'] + c['fw']['H'] + [c['fw']['out']]:
        if a is not None:
            a.setflags(write=False)
    return c


SZ_A, SZ_B = 5, 41   # the two neurons of signed_zero_case


@functools.lru_cache(maxsize=None)
def signed_zero_case(m, n_hidden):
    """exact_case(out_act 0) in which identity input 0 is 2^-14 for every sample, column 16 of W0 is zero except W0[SZ_A, 16] = -2^-14 and
    W0[SZ_B, 16] = +2^-14, and those two rows hold nothing else: their pre-activations are -+2^-28, which round to fp16 -+0 -- both units are dead.
    Returns (case, twin): `twin` is the same case with the two weights zero; it is provably exact, and the restatement gives the same gradients for both
    (asserted), so the case's own results are exact as well: the two products w x = 2^-28 are single addends of their accumulators."""
    base = exact_case(m, n_hidden, 0, seed=7)
    out = []
    for w in (2.0 ** -14, 0.0):
        W = base['W'].copy()
        W0 = W[:W0_N].reshape(64, 32)
        W0[:, 16] = 0.0
        W0[[SZ_A, SZ_B]] = 0.0
        W0[SZ_A, 16], W0[SZ_B, 16] = -w, w
        x16 = base['x16'].copy()
        x16[:, 3] = 2.0 ** -14
        out.append(finish_case(dict(m=m, n_hidden=n_hidden, out_act=0, loss_scale=128.0, n_out_rows=16, W=W, x16=x16, g=base['g'].copy(), y=None, old=None),
                               need_exact=(w == 0.0)))
    case, twin = out
    assert np.array_equal(case['dW'], twin['dW']) and np.array_equal(case['d_in'], twin['d_in']) and np.array_equal(case['fw']['out'], twin['fw']['out'])
    assert np.all(case['fw']['Z'][0][:, SZ_A] == -2.0 ** -28) and np.all(case['fw']['Z'][0][:, SZ_B] == 2.0 ** -28)
    return case, twin


DEAD0, DEAD1 = (3, 30, 63), (0, 17, 62)   # neurons of random_case that are dead for every sample (first / second hidden layer)


@functools.lru_cache(maxsize=None)
def random_case(m, n_hidden, out_act, seed=0):
    """Random fp16 data at realistic magnitudes: Xavier-uniform weights, identity inputs N(0, 0.5), unit directions, gradients N(0, 1e-2) of which every
    seventh row is scaled by 2^-13 (g x 128 is an fp16 subnormal there), an old gradient buffer N(0, 0.1).  Identity input 15 is >= 0.5 and the neurons
    DEAD0 read only it, with weight -1: dead for every sample; with two hidden layers the rows DEAD1 of W1 are -|w|: dead as well."""
    rng = np.random.default_rng([seed, m, n_hidden, out_act, 1])
    shapes = [(64, 32)] + [(64, 64)] * (n_hidden - 1) + [(16, 64)]
    Wl = [(rng.random(s) * 2 - 1) * np.sqrt(6.0 / (s[0] + s[1])) for s in shapes]
    Wl[0][list(DEAD0)] = 0.0
    Wl[0][list(DEAD0), 31] = -1.0
    if n_hidden > 1:
        Wl[1][list(DEAD1)] = -np.abs(Wl[1][list(DEAD1)]) - 2.0 ** -10
    W = h16(np.concatenate([w.reshape(-1) for w in Wl]))
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ident = rng.normal(size=(m, 16)) * 0.5
    ident[:, 15] = np.abs(ident[:, 15]) + 0.5
    x16 = np.concatenate([d * 0.5 + 0.5, ident], 1).astype(np.float16)
    g = rng.normal(size=(m, 16)) * 1e-2
    g[::7] *= 2.0 ** -13
    old = (rng.normal(size=n_weights(n_hidden)) * 0.1).astype(np.float32)
    c = dict(m=m, n_hidden=n_hidden, out_act=out_act, loss_scale=128.0, n_out_rows=16, W=W, x16=x16, g=g.astype(np.float16), old=old, X=encode(x16))
    for a in (W, x16, c['g'], old, c['X']):
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_mlp_grad.py
FWD_M = (1, 31, 32, 33, 129, 65536, 65537)                                    # the forward's tile loop wraps at 512 workgroups x 128 rows
BWD_M = (1, 31, 32, 33, 127, 128, 129, 4097, 32768, 32769, 98337)             # the backward's at 256 x 128; 98 337 = 3 x 32 768 + 33
NETS = ((1, 0), (2, 0), (1, 1), (2, 1))                                       # (n_hidden, out_act)
SHAPES = ((16, 16, 16), (3, 4, 4), (1, 4, 4), (8, 8, 8), (12, 12, 12), (5, 16, 8))   # (n_out_rows, out_ld, n_store)
SHAPE_M = (129, 32769)
LOSS_SCALES = (1.0, 128.0, 1024.0)
MODULE_M = (1, 33, 32769)
SIGNED_ZERO_CASES = ((33, 1), (33, 2), (4097, 1), (4097, 2))


def gpu_exact_cases():
    """keyword sets of every exact_case the GPU file asks for"""
    out = [dict(m=m, n_hidden=nh, out_act=0) for m in FWD_M for nh in (1, 2)]
    out += [dict(m=m, n_hidden=nh, out_act=a) for m in BWD_M for nh, a in NETS]
    out += [dict(m=m, n_hidden=2, out_act=a, n_out_rows=s[0], with_old=True) for m in SHAPE_M for s in SHAPES for a in (0, 1)]
    out += [dict(m=m, n_hidden=2, out_act=a, loss_scale=ls) for m in (129, 4097) for a in (0, 1) for ls in LOSS_SCALES]
    out += [dict(m=m, n_hidden=nh, out_act=a, with_old=True) for m in (129, 32769) for nh, a in NETS]
    out += [dict(m=m, n_hidden=2, out_act=0, g_cols=3) for m in MODULE_M]
    out += [dict(m=m, n_hidden=1, out_act=0, grid=True) for m in MODULE_M]
    seen, uniq = set(), []
    for kw in out:
        key = tuple(sorted(kw.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(kw)
    return uniq
