"""A float64 restatement, an exactness proof and a per-stage error budget for the fused NeRF block (nerficg_amd/csrc/nerf_net.hip: k_nerf_forward;
C ABI group 17, include/nerficg_hip.h; Python: nerficg_amd.nerf.fused_forward).  Plain module: no test functions.  Modelled on tests/mlp_ref.py (read
its docstring first); used by tests/test_nerf_mlp_ref_cpu.py and tests/test_gpu_nerf_fused.py.

The restatement (`forward`, `layer`)
---------------
h16(.) is round-to-nearest-even to fp16; sat(.) clamps to +-65504 (an overflowing conversion gives inf, which sat brings back); weights are sat(h16(w)).
    enc(x)   = [x (if append_input) | per dimension: cos(x 2^k) k < K, sin(x 2^k) k < K], x 2^k the exact product, cos / sin in float64, then h16
    H_1      = sat(relu(h16(b_0 + W_0 enc_pos)))
    H_l+1    = sat(relu(h16(b_l + W_l [H_l | enc_pos if l in skips])))          l = 1 .. L-1   (the encoded position BEHIND the hidden units)
    sigma    = relu(b_s + w_s H_L)                                               (f32 on the device, never fp16)
    F        = sat(h16(b_f + W_f H_L))                                            (no ReLU)
    C_1      = sat(relu(h16(b + W [F | enc_dir])))  ;  C_q+1 = sat(relu(h16(b + W C_q)))  ;  rgb = 1 / (1 + exp(-(b + W C_n)))
Conversion first, then ReLU, then saturation: the order of the kernel.  Everything else is float64.  The stage list, in the order of the kernel's taps
(tap = 1 + index), is STAGES(net) = [enc_pos, enc_dir, H_1 .. H_L, F, C_1 .. C_n]; the two outputs are the stages 'sigma' and 'rgb'.

Exactness (`exact`)
-------------------
The proof of mlp_ref.exact: if every value that is converted to fp16 (encodings, every Z of a hidden, feature or colour stage) is an fp16 number of
magnitude <= 65504 already, and for every f32 accumulator (bias included as one addend) the sum of |addends| stays below 2^24 units, the unit being a
power of two that divides every addend, then no partial sum in any order rounds, and the device equals the restatement BIT FOR BIT: every tap and
sigma.  rgb passes through f32 expf and a division, which no choice of inputs makes exact: it is held to the sigmoid bound below with e_Z = 0 (a few
f32 ulp), while its operand C_n and therefore its pre-activation are covered bit for bit.
Exact cases use K = 0 with append_input (the encoding is the identity) and x = 0 with K = 10 / 4 (cos 0 = 1, sin 0 = 0 exactly: drives every cos
column of the first and the skip layers); weights are sparse with entries +-1 (small dyadics in the heads), biases small integers.

The budget (`stage_budget`; u = 2^-24, gamma(k) = k u / (1 - k u))
----------
One stage at a time, from an operand the DEVICE produced (an exact input: E = 0) to the next one.  K addends:
    e_Z = gamma(K + 2) |W| |A| + |b| u      (products of fp16 numbers are exact in f32; at most K additions on any addend's path with the bias as the
                                            accumulator's start, + 2 of slack; the bias itself is an f32 number the device reads unrounded)
    conversion: rounding is monotone, so the device's operand lies between sat(relu(h16(Z - e_Z))) and sat(relu(h16(Z + e_Z))): the bound is the larger
                distance of the two from the restated operand -- zero unless an fp16 rounding boundary lies within +-e_Z, one ulp or more if it does.
    encodings:  E_ENC = 2^-22 takes the place of e_Z for the sin / cos columns (the kernel's stated bound on |f32 value - float64 function| for
                |x| <= 8, k <= 9; `sincos_model` restates the kernel's f32 sequence, and tests/test_nerf_mlp_ref_cpu.py scans it densely: the bound
                comes from the analysis at the top of csrc/nerf_net.hip, the scan only confirms it); 0 for the appended input, whose conversion
                from f32 is the restatement's own.
    sigma:      relu is 1-Lipschitz: |device - relu(Z)| <= e_Z.
    rgb:        the device value lies in [s(Z - e_Z) (1 - E_SIGMOID), s(Z + e_Z) (1 + E_SIGMOID)], s the float64 sigmoid, E_SIGMOID = 2^-21: expf within
                1 ulp at a relative condition e/(1+e) <= 1, one addition and one correctly rounded division at half an ulp each -- 2 ulp = 2^-22,
                doubled.  f32 range: below 2^-126 the quotient is subnormal, or 0 once expf(-Z) overflows (Z < -88.7), so a lower end
                below 2^-126 is replaced by 0 and the upper end gets 2^-149 (one subnormal step) on top.
No measured constant, no tensor maximum and no excluded element enters.  The float64 restatement's own rounding is 2^-29 of any gamma term.
"""
from __future__ import annotations

import functools

import numpy as np

U32 = 2.0 ** -24
E_ENC = 2.0 ** -22
E_SIGMOID = 2.0 ** -21
H16_MAX = 65504.0

MUTATIONS = ('swap_cos_sin', 'skip_early', 'skip_late', 'enc_in_front', 'drop_bias', 'feature_relu', 'dir_in_front', 'transpose_weight',
             'last_row_neighbour')


def gamma32(k):
    k = np.asarray(k, np.float64)
    return k * U32 / (1.0 - k * U32)


def h16(a):
    with np.errstate(over='ignore'):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def sat(a):
    return np.clip(a, -H16_MAX, H16_MAX)


def relu(h):
    return np.maximum(h, 0.0) + 0.0


def sigmoid(z):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


# ------------------------------------------------------------------------------------------------ the network
def make_net(linears, n_layers, n_color_layers, k_pos, k_dir, append_input, skips):
    """linears: [(W, b)] in the packed order -- initial_layers[0..L-1], density_layer, feature_layer, colour linears, rgb linear."""
    lin = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in linears]
    assert len(lin) == n_layers + 3 + n_color_layers
    return dict(lin=lin, L=int(n_layers), n_color=int(n_color_layers), k_pos=int(k_pos), k_dir=int(k_dir), append=bool(append_input),
                skips=frozenset(int(k) for k in skips if 1 <= int(k) < n_layers), width=lin[n_layers + 1][0].shape[0])


def net_from_block(block):
    from nerficg_amd import nerf
    lin = [(m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy()) for m in nerf._block_linears(block)]
    return make_net(lin, len(block.initial_layers), len(block.color_layers) - 3, block.encoding_position.frequency_factors.numel(),
                    block.encoding_direction.frequency_factors.numel(), block.encoding_position.append_input, block.input_skips)


def block_from_net(net, device='cpu'):
    """A NeRFBlock (f32) holding the net's parameters (they must be f32 numbers for the two to agree)."""
    import torch
    from nerficg_amd import nerf
    block = nerf.NeRFBlock(net['L'], net['n_color'], net['width'], net['k_pos'], net['k_dir'], net['append'], sorted(net['skips']))
    with torch.no_grad():
        for m, (w, b) in zip(nerf._block_linears(block), net['lin']):
            assert tuple(m.weight.shape) == w.shape, (m.weight.shape, w.shape)
            m.weight.copy_(torch.from_numpy(w).float())
            m.bias.copy_(torch.from_numpy(b).float())
    return block.to(device)


def n_enc(k, append):
    return 6 * k + (3 if append else 0)


def STAGES(net):
    w = net['width']
    return ([('enc_pos', n_enc(net['k_pos'], net['append'])), ('enc_dir', n_enc(net['k_dir'], net['append']))]
            + [(f'H_{l}', w) for l in range(1, net['L'] + 1)] + [('F', w)] + [(f'C_{q}', w // 2) for q in range(1, net['n_color'] + 1)])


def encode_f64(x, k, append, swap=False):
    """(values before the fp16 conversion, is-a-sin/cos-column mask); x: (M, 3) f32 numbers"""
    x = np.asarray(x, np.float32).astype(np.float64)
    f = x[:, :, None] * (2.0 ** np.arange(k))[None, None, :]      # exact: a power of two times an f32 number
    parts = (np.sin(f), np.cos(f)) if swap else (np.cos(f), np.sin(f))
    enc = np.concatenate(parts, axis=-1).reshape(x.shape[0], -1)
    trig = np.ones(enc.shape[1], bool)
    if append:
        enc, trig = np.concatenate([x, enc], axis=1), np.concatenate([np.zeros(3, bool), trig])
    return enc, trig


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)   # f32 operands: the product is exact in f64


def sincos_model(a):
    """nerf_sincos of csrc/nerf_net.hip step by step in f32 (every fmaf rounded once): -> (sin, cos) as f32 arrays"""
    f32 = np.float32
    a = np.asarray(a, f32)
    c = lambda v: np.full_like(a, v)
    n = np.rint((a * f32(0.636619772)).astype(f32)).astype(f32)
    r = _fma32(-n, c(1.5703125), a)
    r = _fma32(-n, c(4.837512969970703125e-4), r)
    r = _fma32(-n, c(7.54978995489188216e-8), r)
    z = (r * r).astype(f32)
    ps = _fma32(_fma32(c(-1.9515295891e-4), z, c(8.3321608736e-3)), z, c(-1.6666654611e-1))
    s = _fma32((ps * z).astype(f32), r, r)
    pc = _fma32(_fma32(c(2.443315711809948e-5), z, c(-1.388731625493765e-3)), z, c(4.166664568298827e-2))
    co = _fma32(pc, (z * z).astype(f32), _fma32(c(-0.5), z, c(1.0)))
    q = n.astype(np.int64) & 3
    return (np.where(q == 0, s, np.where(q == 1, co, np.where(q == 2, -s, -co))), np.where(q == 0, co, np.where(q == 1, -s, np.where(q == 2, -co, s))))


def _stage_inputs(net, name):
    """(index of the linear, names of the operands that are concatenated, activation)"""
    L, n = net['L'], net['n_color']
    if name == 'sigma':
        return L, [f'H_{L}'], 'out_relu'
    if name == 'F':
        return L + 1, [f'H_{L}'], 'none'
    if name == 'rgb':
        return L + 2 + n, [f'C_{n}'], 'sigmoid'
    kind, idx = name.split('_')
    idx = int(idx)
    if kind == 'H':
        if idx == 1:
            return 0, ['enc_pos'], 'relu'
        return idx - 1, [f'H_{idx - 1}'] + (['enc_pos'] if (idx - 1) in net['skips'] else []), 'relu'
    assert kind == 'C'
    return (L + 2, ['F', 'enc_dir'], 'relu') if idx == 1 else (L + 1 + idx, [f'C_{idx - 1}'], 'relu')


def stage_operands(net, name):
    return _stage_inputs(net, name)[1]


def layer(net, name, operands, rounding=True, mut=None):
    """One stage from its fp16 operands (dict name -> (M, width) array) -> dict(Z, out, A, W, b).  `out` is the next operand, or sigma / rgb."""
    li, names, act = _stage_inputs(net, name)
    W, b = net['lin'][li]
    if rounding:
        W = sat(h16(W))
    if mut == 'transpose_weight' and name == 'H_2':
        W = W.copy()
        W[:32, :32] = W[:32, :32].T.copy()
    if mut == 'drop_bias' and name == f'H_{net["L"]}':
        b = np.zeros_like(b)
    A = [np.asarray(operands[n], np.float64) for n in names]
    if (mut == 'enc_in_front' and name.startswith('H_') and len(A) == 2) or (mut == 'dir_in_front' and name == 'C_1'):
        A = A[::-1]
    A = np.concatenate(A, axis=1)
    Z = A @ W.T + b
    rd = (lambda a: sat(h16(a))) if rounding else (lambda a: a)
    if act == 'relu' or (mut == 'feature_relu' and name == 'F'):
        out = sat(relu(h16(Z))) if rounding else relu(Z)
    elif act == 'none':
        out = rd(Z)
    elif act == 'out_relu':
        out = relu(Z)
    else:
        out = sigmoid(Z)
    return dict(Z=Z, out=out, A=A, W=W, b=b)


def forward(net, positions, directions, rounding=True, mut=None, tile_rows=128):
    """dict: every stage of STAGES plus 'sigma' (M,) and 'rgb' (M, 3).  mut: one of MUTATIONS -- a deliberately wrong restatement."""
    assert mut is None or mut in MUTATIONS
    pos, dirs = np.asarray(positions, np.float32).copy(), np.asarray(directions, np.float32)
    m = pos.shape[0]
    if mut == 'last_row_neighbour' and m % tile_rows != 0 and m > 1:
        pos[m - 1] = pos[m - 2]
    rd = h16 if rounding else (lambda a: a)
    out = {'enc_pos': rd(encode_f64(pos, net['k_pos'], net['append'], swap=mut == 'swap_cos_sin')[0]),
           'enc_dir': rd(encode_f64(dirs, net['k_dir'], net['append'], swap=mut == 'swap_cos_sin')[0])}
    q = (lambda w: sat(h16(w))) if rounding else (lambda w: w)
    shift = {'skip_early': -1, 'skip_late': 1}.get(mut, 0)
    for l in range(net['L']):                              # l: index of the linear, its stage is H_(l+1)
        name = f'H_{l + 1}'
        if shift and l >= 1:
            # the encoded position's weight block of skip layer k is applied at layer k + shift; every layer keeps its hidden block
            W, b = net['lin'][l]
            Z = out[f'H_{l}'] @ q(W)[:, :net['width']].T + b
            if (l - shift) in net['skips']:
                Z = Z + out['enc_pos'] @ q(net['lin'][l - shift][0])[:, net['width']:].T
            out[name] = sat(relu(h16(Z))) if rounding else relu(Z)
        else:
            out[name] = layer(net, name, out, rounding, mut)['out']
    for name in ['sigma', 'F'] + [f'C_{q}' for q in range(1, net['n_color'] + 1)] + ['rgb']:
        out[name] = layer(net, name, out, rounding, mut)['out']
    out['sigma'] = out['sigma'][:, 0]
    return out


# ------------------------------------------------------------------------------------------------ exactness
def _bits(a):
    s = np.abs(np.asarray(a, np.float64)) * 2.0 ** 40
    n = s.astype(np.int64)
    assert np.all(n == s), 'value finer than 2^-40'
    return n


def _low(n):
    return np.where(n == 0, np.inf, (n & -n).astype(np.float64) * 2.0 ** -40)


def _acc_ratio(A, Wt, extra):
    """accumulators A @ Wt + extra[None, :]: sum |addends| / (2^24 unit), unit = minlow(row of A) minlow(column of Wt), and the low bit of extra"""
    unit = np.outer(_low(np.bitwise_or.reduce(_bits(A), axis=1)), _low(np.bitwise_or.reduce(_bits(Wt), axis=0)))
    unit = np.minimum(unit, _low(_bits(extra))[None, :])
    s = np.abs(A) @ np.abs(Wt) + np.abs(extra)[None, :]
    return float(np.max(np.where(s > 0, s / (2.0 ** 24 * np.where(np.isfinite(unit), unit, 1.0)), 0.0), initial=0.0))


def exact(net, positions, directions, fw=None):
    """(ok, fp16_max, acc_max): both conditions of the module docstring for every stage."""
    fw = forward(net, positions, directions) if fw is None else fw
    ok = all(bool(np.all(sat(h16(w)) == w)) for w, _ in net['lin'])
    fp16_max, acc = 0.0, []
    for name, k in (('enc_pos', net['k_pos']), ('enc_dir', net['k_dir'])):
        raw = encode_f64(positions if name == 'enc_pos' else directions, k, net['append'])[0]
        ok = ok and bool(np.all(h16(raw) == raw))
    for name in [n for n, _ in STAGES(net)[2:]] + ['sigma', 'rgb']:
        st = layer(net, name, fw)
        if name not in ('sigma', 'rgb'):
            ok = ok and bool(np.all(h16(st['Z']) == st['Z'])) and bool(np.all(np.abs(st['Z']) <= H16_MAX))
            fp16_max = max(fp16_max, float(np.abs(st['Z']).max(initial=0.0)))
        acc.append(_acc_ratio(st['A'], st['W'].T, st['b']))
    return bool(ok and max(acc) < 1.0), fp16_max, max(acc)


# ------------------------------------------------------------------------------------------------ budget
def _conv_bound(z, e, ref, act):
    lo, hi = h16(z - e), h16(z + e)
    if act:
        lo, hi = relu(lo), relu(hi)
    lo, hi = sat(lo), sat(hi)
    return np.maximum(np.abs(lo - ref), np.abs(hi - ref))


def encoding_budget(x, k, append):
    """(restated fp16 operand, per-element bound) of an encoding tap"""
    raw, trig = encode_f64(x, k, append)
    ref = h16(raw)
    return ref, _conv_bound(raw, np.where(trig, E_ENC, 0.0)[None, :], ref, act=False)


def stage_budget(net, name, operands):
    """(ref, bound) for a hidden / feature / colour stage and for sigma: |device - ref| <= bound per element;
    (ref, (lo, hi)) for rgb: the device value must lie in [lo, hi]."""
    st = layer(net, name, operands)
    k = st['A'].shape[1]
    eZ = gamma32(k + 2) * (np.abs(st['A']) @ np.abs(st['W']).T) + np.abs(st['b'])[None, :] * U32
    _, _, act = _stage_inputs(net, name)
    if act == 'out_relu':
        return st['out'], eZ
    if act == 'sigmoid':
        lo, hi = sigmoid(st['Z'] - eZ), sigmoid(st['Z'] + eZ)
        return st['out'], (np.where(lo < 2.0 ** -126, 0.0, lo * (1.0 - E_SIGMOID)), hi * (1.0 + E_SIGMOID) + 2.0 ** -149)
    return st['out'], _conv_bound(st['Z'], eZ, st['out'], act == 'relu')


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


def chained_check(net, positions, directions, got):
    """The chained budget on a set of taps `got` (dict: every stage of STAGES, 'sigma', 'rgb' -- a device's, or a mutant restatement's): each stage
    against `layer(stage, got's own operands)`.  -> {stage: (elements over their bound, worst error / bound)}"""
    res = {}
    for name, k, x in (('enc_pos', net['k_pos'], positions), ('enc_dir', net['k_dir'], directions)):
        ref, bound = encoding_budget(x, k, net['append'])
        ratio, over = judge(got[name], ref, bound)
        res[name] = (over, ratio)
    for name in [n for n, _ in STAGES(net)[2:]] + ['sigma', 'rgb']:
        ref, bound = stage_budget(net, name, got)
        g = np.asarray(got[name], np.float64).reshape(ref.shape)
        if name == 'rgb':
            res[name] = (judge_interval(g, bound), float('nan'))
        else:
            ratio, over = judge(g, ref, bound)
            res[name] = (over, ratio)
    return res


def exact_check(fw, got):
    """Stages of `got` that differ from the restatement `fw` of an exact case: bit for bit, except rgb (the sigmoid bound at e_Z = 0)."""
    bad = [n for n in fw if n != 'rgb' and not np.array_equal(np.asarray(got[n], np.float64).reshape(fw[n].shape), fw[n])]
    g = np.asarray(got['rgb'], np.float64)
    if not bool(np.all((g >= fw['rgb'] * (1.0 - E_SIGMOID)) & (g <= fw['rgb'] * (1.0 + E_SIGMOID)))):
        bad.append('rgb')
    return bad


# ------------------------------------------------------------------------------------------------ cases
def _sparse(rng, rows, cols, nnz, values=(-1.0, 1.0)):
    W = np.zeros((rows, cols))
    for r in range(rows):
        W[r, rng.choice(cols, size=min(nnz, cols), replace=False)] = rng.choice(values, size=min(nnz, cols))
    return W


@functools.lru_cache(maxsize=None)
def exact_net(width, family, seed=0):
    """family 'identity': K = 0, append_input, L = 8, skips (5,), two colour layers.  family 'zero': K = 10 / 4, skips (2, 5), one colour layer (inputs 0)."""
    rng = np.random.default_rng([seed, width, family == 'zero'])
    if family == 'identity':
        L, n_color, k_pos, k_dir, skips = 8, 2, 0, 0, (5,)
    else:
        L, n_color, k_pos, k_dir, skips = 8, 1, 10, 4, (2, 5)
    n_pos, n_dir, half = n_enc(k_pos, True), n_enc(k_dir, True), width // 2
    ib = lambda n, hi=2: rng.integers(0, hi + 1, size=n).astype(np.float64)
    lin = [(_sparse(rng, width, n_pos, 2), ib(width))]
    for l in range(1, L):
        W = _sparse(rng, width, width, 2)
        if l in skips:
            W = np.concatenate([W, _sparse(rng, width, n_pos, 1)], axis=1)
        lin.append((W, ib(width, 1)))
    lin.append((_sparse(rng, 1, width, 8, (-0.25, 0.25, 0.5)), ib(1)))
    lin.append((_sparse(rng, width, width, 2), ib(width, 3) - 1.0))
    lin.append((np.concatenate([_sparse(rng, half, width, 2), _sparse(rng, half, n_dir, 1)], axis=1), ib(half, 1)))
    for _ in range(n_color - 1):
        lin.append((_sparse(rng, half, half, 2), ib(half, 1)))
    lin.append((_sparse(rng, 3, half, 6, (-0.0625, 0.0625, 0.125)), ib(3, 1) - 0.5))
    return make_net(lin, L, n_color, k_pos, k_dir, True, skips)


def exact_inputs(m, family, seed=0):
    rng = np.random.default_rng([seed, m, 7])
    if family == 'zero':
        return np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
    return (rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 3.0], size=(m, 3)).astype(np.float32),
            rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], size=(m, 3)).astype(np.float32))


def random_inputs(m, seed=0):
    """positions in [-4, 4]^3, unit directions"""
    rng = np.random.default_rng([seed, m, 11])
    d = rng.normal(size=(m, 3))
    return rng.uniform(-4.0, 4.0, size=(m, 3)).astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def f32_stage_shuffled(net, name, operands, rng):
    """An f32 emulation of one stage: the bias and the K products added one by one in a random order, every partial sum rounded to f32; then the
    stage's conversion.  What a device with ANY summation order may return."""
    st = layer(net, name, operands)
    A, W = st['A'].astype(np.float32), st['W'].astype(np.float32)
    k = A.shape[1]
    order = rng.permutation(k + 1)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for j in order:
        acc = (acc + (st['b'].astype(np.float32)[None, :] if j == k else A[:, j:j + 1] * W[None, :, j])).astype(np.float32)
    z = acc.astype(np.float64)
    _, _, act = _stage_inputs(net, name)
    if act == 'out_relu':
        return relu(z)
    if act == 'sigmoid':
        with np.errstate(over='ignore'):
            return (np.float32(1.0) / (np.float32(1.0) + np.exp(-acc))).astype(np.float64)
    return sat(relu(h16(z))) if act == 'relu' else sat(h16(z))
