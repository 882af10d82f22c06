"""GPU: the fully fused MLP kernels (nerficg_amd/csrc/ngp_net.hip: k_nwie_fwd, k_nwie_bwd) through the C ABI and through
nerficg_amd.tinycudann.NetworkWithInputEncoding against the float64 restatement of tests/mlp_ref.py.

Exact cases: inputs for which mlp_ref.exact proves that no f32 addition and no fp16 conversion can round, whatever the order of the sums -- the MFMA
chains, the LDS reduction and the atomics must then give the restatement's value bit for bit, compared with `==` (so -0.0 equals 0.0) and no tolerance:
every batch size at which the tile loops take another turn, every legal output shape, three loss scales, a non-zero gradient buffer, sentinel rows and
columns around everything that is written.  Budget cases: random fp16 data, every element inside its own bound (derivation in mlp_ref's docstring);
each prints its worst error / budget.  The saved state between the two calls stays private: nothing here decodes it."""
import numpy as np
import pytest
import torch

from nerficg_amd import _lib
from tests import mlp_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
OUT_SENT, F_SENT, TAIL = -777.0, 12345.0, 64


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a, order='C'))   # (a copy: the cached cases are read-only)
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _junk(m, n):
    """finite non-zero integers of both signs"""
    i, j = np.arange(m)[:, None], np.arange(n)[None, :]
    return (((i + 2 * j) % 5 + 1) * np.where((i + j) % 2, -1.0, 1.0)).astype(np.float16)


def run(c, shape=(16, 16, 16), pair_major=0, old=None, junk=False, y=None, backward=True):
    """nrc_nwie_forward (encoding 1, save buffers of nrc_nwie_save_rows(M) rows) and nrc_nwie_backward on that state.  shape = (n_out_rows, out_ld,
    n_store); y: the `out` handed to the backward (None: the forward's own).  Every output buffer carries TAIL sentinel rows behind the M-th (the
    pair-major d_in, whose layout has no rows behind M, as many floats behind its end)."""
    lib = _lib.load()
    nor, out_ld, n_store = shape
    m, nh, act, ls = c['m'], c['n_hidden'], c['out_act'], c['loss_scale']
    rows = int(lib.nrc_nwie_save_rows(m))
    assert rows == (m + 31) // 32 * 32
    w16, x = T(c['W'], torch.float16), T(c['x16'])
    out = torch.full((m + TAIL, out_ld), OUT_SENT, dtype=torch.float16, device=DEV)
    save_in = torch.empty(rows, 32, dtype=torch.float16, device=DEV)
    save_acts = torch.empty(nh, rows, 64, dtype=torch.float16, device=DEV)
    st = _lib.stream_of(out)
    _lib.check(lib.nrc_nwie_forward(1, _lib.ptr(x), 19, m, _lib.ptr(w16), None, 1, 4, 2, 2.0, nh, act, nor, _lib.ptr(out), out_ld, n_store,
                                    _lib.ptr(save_in), _lib.ptr(save_acts), None, st), 'nwie_forward')
    res = {}
    if backward:
        g = np.array(c['g'][:, :out_ld])
        if junk:
            g[:, nor:] = _junk(m, out_ld)[:, nor:]
        g16 = T(g)
        ybuf = out if y is None else T(np.asarray(y, np.float16)[:, :out_ld])
        nw = R.n_weights(nh)
        dW = torch.full((nw + TAIL,), F_SENT, dtype=torch.float32, device=DEV)
        dW[:nw] = 0.0 if old is None else T(old)
        d_in = torch.full(((m + TAIL) * 32,), F_SENT, dtype=torch.float32, device=DEV)
        _lib.check(lib.nrc_nwie_backward(m, _lib.ptr(w16), nh, act, nor, _lib.ptr(g16), _lib.ptr(ybuf), out_ld, _lib.ptr(save_in), _lib.ptr(save_acts),
                                         float(ls), _lib.ptr(dW), _lib.ptr(d_in), pair_major, st), 'nwie_backward')
        torch.cuda.synchronize()
        dW, d_in = dW.cpu().numpy(), d_in.cpu().numpy()
        res.update(dW=dW[:nw], dW_tail=dW[nw:], d_in_tail=d_in[32 * m:])
        res['d_in'] = d_in[:32 * m].reshape(16, m, 2).transpose(1, 0, 2).reshape(m, 32) if pair_major else d_in[:32 * m].reshape(m, 32)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    res.update(out=o[:m, :n_store], out_cols_behind=o[:m, n_store:], out_tail=o[m:])
    return res


def _same(got, want, what):
    """`==` on every element (array_equal: -0.0 equals 0.0, NaN equals nothing)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {k}: got {got[k]!r}, want {want[k]!r}')


def _check_sentinels(r, what):
    assert np.all(r['out_tail'] == np.float16(OUT_SENT)) and np.all(r['out_cols_behind'] == np.float16(OUT_SENT)), f'{what}: output written outside [0, M) x [0, n_store)'
    if 'dW' in r:
        assert np.all(r['dW_tail'] == np.float32(F_SENT)), f'{what}: gradient buffer written behind its end'
        assert np.all(r['d_in_tail'] == np.float32(F_SENT)), f'{what}: d_in written behind row M'


def _check_backward(c, r, what):
    _same(r['dW'], c['dW'], f'{what}: dW')
    _same(r['d_in'], c['d_in'], f'{what}: d_in')
    _check_sentinels(r, what)


# ------------------------------------------------------------------------------------------------ exact cases, C ABI
@pytest.mark.parametrize('n_hidden', [1, 2])
@pytest.mark.parametrize('m', R.FWD_M)
def test_forward_exact(m, n_hidden):
    c = R.exact_case(m, n_hidden, 0)
    r = run(c, shape=(16, 20, 16), backward=False)     # out_ld 20: four columns behind n_store that must keep their sentinel
    _same(r['out'], c['fw']['out'], f'forward m {m}')
    assert np.count_nonzero(c['fw']['out'][-1]) > 0
    _check_sentinels(r, f'forward m {m}')


@pytest.mark.parametrize('n_hidden,out_act', R.NETS)
@pytest.mark.parametrize('m', R.BWD_M)
def test_backward_exact(m, n_hidden, out_act):
    c = R.exact_case(m, n_hidden, out_act)
    assert np.count_nonzero(c['d_in'][-1]) > 0 and np.count_nonzero(c['dW']) > 0   # the last row is live: a dropped tail is seen
    for pair_major in (0, 1):
        r = run(c, pair_major=pair_major, y=c['y'])
        _check_backward(c, r, f'backward m {m} pair_major {pair_major}')
        if not out_act:
            _same(r['out'], c['fw']['out'], 'out')


@pytest.mark.parametrize('out_act', [0, 1])
@pytest.mark.parametrize('shape', R.SHAPES)
@pytest.mark.parametrize('m', R.SHAPE_M)
def test_output_shapes_exact(m, shape, out_act):
    """(n_out_rows, out_ld, n_store): the 16-byte row path (out_ld 16), the scalar path (4, 8, 12), Wout rows behind n_out_rows read as zero.  The
    gradient buffer starts from an integer pattern: the rows of Wout's gradient at and behind n_out_rows must keep the caller's BITS, and junk in the
    d_out columns at and behind n_out_rows must change nothing."""
    nor, out_ld, n_store = shape
    c = R.exact_case(m, 2, out_act, n_out_rows=nor, with_old=True)
    r = run(c, shape=shape, old=c['old'], junk=True, y=c['y'])
    what = f'shape {shape} m {m} out_act {out_act}'
    _check_backward(c, r, what)
    wo = slice(R.W0_N + R.WH_N + nor * 64, None)
    assert np.array_equal(r['dW'][wo].view(np.int32), np.asarray(c['old'])[wo].view(np.int32)), f'{what}: gradient rows behind n_out_rows touched'
    if out_act:
        assert np.all(r['out'][:, nor:] == np.float16(0.5))          # sigmoid(0) of the rows that read as zero
    else:
        _same(r['out'], c['fw']['out'][:, :n_store], f'{what}: out')
        assert not c['fw']['out'][:, nor:].any()


@pytest.mark.parametrize('out_act', [0, 1])
@pytest.mark.parametrize('loss_scale', R.LOSS_SCALES)
def test_loss_scale_exact(loss_scale, out_act):
    """the same integer gradients k / loss_scale: every result is the one of loss scale 128, bit for bit"""
    for m in (129, 4097):
        c, c128 = R.exact_case(m, 2, out_act, loss_scale=loss_scale), R.exact_case(m, 2, out_act, loss_scale=128.0)
        s = 128.0 / loss_scale      # gradients are 1 / loss_scale of an integer: results scale with them
        assert np.array_equal(c['dW'], c128['dW'] * s) and np.array_equal(c['d_in'], c128['d_in'] * s) and np.count_nonzero(c['dW']) > 1000
        _check_backward(c, run(c, y=c['y']), f'loss scale {loss_scale} m {m}')


@pytest.mark.parametrize('n_hidden,out_act', R.NETS)
@pytest.mark.parametrize('m', [129, 32769])
def test_accumulates_onto_the_callers_gradient_exact(m, n_hidden, out_act):
    c = R.exact_case(m, n_hidden, out_act, with_old=True)
    zero = R.backward(c['fw'], c['W'], c['g'], c['y'], c['loss_scale'], n_hidden, out_act)[0]
    assert np.array_equal(c['dW'], zero + c['old']) and np.count_nonzero(c['old']) > 0.8 * c['old'].size
    _check_backward(c, run(c, old=c['old'], y=c['y'], pair_major=1), f'accumulate m {m}')


def test_two_calls_give_the_same_bits():
    for c in (R.exact_case(32769, 2, 1), R.random_case(32769, 2, 1)):
        a, b = run(c, y=c.get('y'), pair_major=1), run(c, y=c.get('y'), pair_major=1)
        assert a['out'].tobytes() == b['out'].tobytes() and a['d_in'].tobytes() == b['d_in'].tobytes()
        if 'dW' in c:    # the exact case: the sums cannot depend on the order of the atomics.  (Random data: they may, in the last bits.)
            assert a['dW'].tobytes() == b['dW'].tobytes()


@pytest.mark.parametrize('m,n_hidden', R.SIGNED_ZERO_CASES)
def test_pre_activations_that_round_to_signed_zero_are_dead(m, n_hidden):
    """W0[a, 16] = -2^-14, W0[b, 16] = +2^-14, identity input 0 = 2^-14: pre-activations -+2^-28 -> fp16 -+0.  H = max(fp16(Z), +0), alive iff H > 0:
    both units are dead -- no weight gradient in their rows, no contribution to d_in, and (two hidden layers) none in their columns of dW1."""
    c, _ = R.signed_zero_case(m, n_hidden)
    a, b = R.SZ_A, R.SZ_B
    for pair_major in (0, 1):
        r = run(c, pair_major=pair_major)
        dW0 = r['dW'][:R.W0_N].reshape(64, 32)
        assert not dW0[a].any(), f'unit a (fp16 -0) passes its gradient: {np.count_nonzero(dW0[a])} entries of its dW0 row are set'
        assert not dW0[b].any(), f'unit b (fp16 +0) passes its gradient: {np.count_nonzero(dW0[b])} entries of its dW0 row are set'
        if n_hidden == 2:
            dW1 = r['dW'][R.W0_N:R.W0_N + R.WH_N].reshape(64, 64)
            assert not dW1[:, a].any() and not dW1[:, b].any()
        _check_backward(c, r, f'signed zero m {m}')     # d_in carries nothing of rows a and b of W0 (column 16 would show +-2^-14 dZ0)
        _same(r['out'], c['fw']['out'], 'out')


# ------------------------------------------------------------------------------------------------ exact cases, module level
def _net(tcnn, n_in, n_out, enc, n_hidden):
    cfg = {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': 'None', 'n_neurons': 64, 'n_hidden_layers': n_hidden}
    return tcnn.NetworkWithInputEncoding(n_in, n_out, enc, cfg, seed=3).to(DEV)


@pytest.mark.parametrize('m', R.MODULE_M)
def test_module_sh_identity_network_exact(m):
    import nerficg_amd.tinycudann as tcnn
    enc = {'otype': 'Composite', 'nested': [{'n_dims_to_encode': 3, 'otype': 'SphericalHarmonics', 'degree': 4}, {'otype': 'Identity'}]}
    net = _net(tcnn, 19, 3, enc, 2)
    c = R.exact_case(m, 2, 0, g_cols=3)
    assert net.loss_scale == c['loss_scale'] and net.params.numel() == c['W'].size
    with torch.no_grad():
        net.params.copy_(T(c['W'], torch.float32))
    x = T(c['x16'], torch.float32).requires_grad_(True)     # fp16 numbers in f32: x.grad comes back in f32, unrounded
    out = net(x)
    _same(out.detach().cpu().numpy(), c['fw']['out'][:, :3], f'module out m {m}')
    out.backward(T(c['g'][:, :3]))
    _same(net.params.grad.cpu().numpy(), net._grad_to_master(T(c['dW'], torch.float32)).cpu().numpy().astype(np.float64), f'module params.grad m {m}')
    gx = x.grad.cpu().numpy()
    assert not gx[:, :3].any()
    _same(gx[:, 3:], c['d_in'][:, 16:], f'module x.grad m {m}')


@pytest.mark.parametrize('m', R.MODULE_M)
def test_module_grid_network_exact(m):
    """16 x 2 hash grid whose table is constant per level and feature, every position the origin: fmaf(scale, 0, 0.5) = 0.5 gives all eight corner
    weights 1/8 on every level, so the encoded features are the table's constants whatever the encoder's arithmetic.  The MLP part only."""
    import nerficg_amd.tinycudann as tcnn
    pls = float(np.exp(np.log(2048 * 1.0 / 16) / 15))
    enc = {'otype': 'Grid', 'type': 'Hash', 'n_levels': 16, 'n_features_per_level': 2, 'log2_hashmap_size': 19, 'base_resolution': 16,
           'per_level_scale': pls, 'interpolation': 'Linear'}
    net = _net(tcnn, 3, 16, enc, 1)
    c = R.exact_case(m, 1, 0, grid=True)
    n_mlp = net._n_kernel_mlp
    assert n_mlp == c['W'].size == net.n_mlp_params
    with torch.no_grad():
        net.params[:n_mlp] = T(c['W'], torch.float32)
        table = net.params[n_mlp:].view(-1, 2)
        offs = net.grid_offsets
        for l in range(16):
            table[offs[l]:offs[l + 1]] = T(c['X'][0, 2 * l:2 * l + 2], torch.float32)
    out = net(torch.zeros(m, 3, device=DEV))
    _same(out.detach().cpu().numpy(), c['fw']['out'], f'grid module out m {m}')
    out.backward(T(c['g']))
    _same(net.params.grad[:n_mlp].cpu().numpy(), c['dW'], f'grid module params.grad m {m}')


# ------------------------------------------------------------------------------------------------ budget cases
@pytest.mark.parametrize('n_hidden,out_act', R.NETS)
@pytest.mark.parametrize('m', [33, 4097, 32769])
def test_random_data_inside_the_budget(m, n_hidden, out_act):
    c = R.random_case(m, n_hidden, out_act)
    old = c['old'] if m == 4097 else None
    assert np.any((c['g'] != 0) & (np.abs(c['g'].astype(np.float64)) * 128.0 < 2.0 ** -14))     # g x loss_scale an fp16 subnormal
    for pair_major in (0, 1):
        r = run(c, pair_major=pair_major, old=old)
        b = R.budget(c['X'], c['W'], c['g'], r['out'], c['loss_scale'], n_hidden, out_act, old=old, E_X=R.sh_input_bound(c['x16'], c['X']))
        what = f'random m {m} n_hidden {n_hidden} out_act {out_act} pair_major {pair_major}'
        _check_sentinels(r, what)
        bad = R.judge_interval(r['out'], b['out'])
        e_out = np.maximum(np.abs(b['out'][0] - b['out_ref']), np.abs(b['out'][1] - b['out_ref']))
        (r_o, _), (r_w, over_w), (r_i, over_i) = R.judge(r['out'], b['out_ref'], e_out), R.judge(r['dW'], b['dW_ref'], b['dW']), R.judge(r['d_in'], b['d_in_ref'], b['d_in'])
        print(f'{what}: worst error / budget out {r_o:.3f}, dW {r_w:.3f}, d_in {r_i:.3f}')
        assert bad == 0 and over_w == 0 and over_i == 0, f'{what}: over budget: {bad} outputs, {over_w} weight gradients (worst {r_w:.3g} x), {over_i} input gradients (worst {r_i:.3g} x)'
        # neurons that are dead for every sample: their rows keep the caller's bits (zero budget -- asserted here by name)
        start = np.zeros(R.n_weights(n_hidden), np.float32) if old is None else old
        dW0, s0 = r['dW'][:R.W0_N].reshape(64, 32), start[:R.W0_N].reshape(64, 32)
        assert np.array_equal(dW0[list(R.DEAD0)], s0[list(R.DEAD0)])
        if n_hidden == 2:
            dW1, s1 = r['dW'][R.W0_N:R.W0_N + R.WH_N].reshape(64, 64), start[R.W0_N:R.W0_N + R.WH_N].reshape(64, 64)
            assert np.array_equal(dW1[list(R.DEAD1)], s1[list(R.DEAD1)]) and np.array_equal(dW1[:, list(R.DEAD0)], s1[:, list(R.DEAD0)])
