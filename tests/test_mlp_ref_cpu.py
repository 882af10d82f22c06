"""CPU: the float64 restatement of the fully fused MLP (tests/mlp_ref.py) against the serial f32 C oracle (bit for bit on provably exact inputs, inside the
per-element budget on random ones), against central differences of its own forward, and against deliberately wrong versions of itself -- the evidence
that tests/test_gpu_mlp_grad.py, which holds the HIP kernels to the same restatement, would notice a subtly wrong kernel."""
import itertools

import numpy as np
import pytest

import oracle
from tests import mlp_ref as R


def _oracle(c, X, y=None):
    """(out, acts, dW, d_in) of oracle.mlp_fw / mlp_bw as the existing GPU tests call them: d_out x loss_scale in, results / loss_scale out"""
    nh, act, ls = c['n_hidden'], c['out_act'], np.float32(c['loss_scale'])
    W32, X32 = c['W'].astype(np.float32), X.astype(np.float32)
    out, acts = oracle.mlp_fw(X32, W32, n_hidden=nh, out_act=act, want_acts=True)
    y32 = out if y is None else np.asarray(y, np.float32)
    dW, d_in = oracle.mlp_bw(X32, W32, y32, acts, c['g'].astype(np.float32) * ls, n_hidden=nh, out_act=act)
    return out, acts, dW / ls, d_in / ls


def test_sh_columns_of_the_exact_cases_round_like_float64():
    d01 = np.array(list(itertools.product([0.0, 0.5, 1.0], repeat=3)))
    got = oracle.sh4_encode(d01.astype(np.float32)).astype(np.float64)
    assert np.array_equal(got, R.h16(R.sh4_f64(d01)))
    used = np.unique(np.concatenate([R.exact_case(m, 2, 0)['x16'][:, :3] for m in (129, 4097)]).astype(np.float64), axis=0)
    assert all(any(np.array_equal(u, d) for d in d01) for u in used) and len(used) == 27


@pytest.mark.parametrize('m', [33, 4097])
@pytest.mark.parametrize('n_hidden,out_act', [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_restatement_equals_serial_f32_oracle_on_exact_cases(m, n_hidden, out_act):
    c = R.exact_case(m, n_hidden, out_act)
    out, acts, dW, d_in = _oracle(c, c['X'], c['y'])
    if not out_act:   # (the sigmoid's fp16 output is not an exact quantity: the oracle's f32 expf against float64 is the budget's subject)
        assert np.array_equal(out, c['fw']['out'])
    for l in range(n_hidden):
        assert np.array_equal(acts[l], c['fw']['H'][l]), l
    assert np.count_nonzero(c['dW']) > 1000 and np.count_nonzero(c['d_in']) > 16
    assert np.array_equal(dW, c['dW'])
    assert np.array_equal(d_in, c['d_in'])


@pytest.mark.parametrize('n_hidden,out_act', [(1, 0), (2, 1)])
def test_unrounded_restatement_against_central_differences(n_hidden, out_act):
    """L = sum(out * g): dL/dW and dL/dX of the restatement with every rounding off (and loss_scale 8, which must cancel) against central differences
    of its forward in float64.  Smooth weights; a step of 1e-6 crosses a ReLU kink with negligible probability (the pre-activations are O(0.3))."""
    rng = np.random.default_rng(n_hidden)
    m, nw = 7, R.n_weights(n_hidden)
    W, X, g = rng.normal(size=nw) * 0.3, rng.normal(size=(m, 32)), rng.normal(size=(m, 16))

    def loss(W_, X_):
        return float(np.sum(R.forward(X_, W_, n_hidden, out_act, rounding=False)['out'] * g))
    fw = R.forward(X, W, n_hidden, out_act, rounding=False)
    dW, d_in = R.backward(fw, W, g, fw['out'], 8.0, n_hidden, out_act, rounding=False)
    h = 1e-6
    for k in rng.choice(nw, size=60, replace=False):
        e = np.zeros(nw)
        e[k] = h
        fd = (loss(W + e, X) - loss(W - e, X)) / (2 * h)
        assert abs(fd - dW[k]) <= 1e-7 * max(1.0, abs(fd)), (k, fd, dW[k])
    for i, k in zip(rng.integers(0, m, size=20), rng.integers(0, 32, size=20)):
        e = np.zeros((m, 32))
        e[i, k] = h
        fd = (loss(W, X + e) - loss(W, X - e)) / (2 * h)
        assert abs(fd - d_in[i, k]) <= 1e-7 * max(1.0, abs(fd)), (i, k, fd, d_in[i, k])


@pytest.mark.parametrize('n_hidden,out_act', [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_serial_f32_oracle_lies_inside_the_budget_on_random_data(n_hidden, out_act):
    c = R.random_case(4097, n_hidden, out_act)
    out, acts, dW, d_in = _oracle(c, c['X'])
    b = R.budget(c['X'], c['W'], c['g'], out, c['loss_scale'], n_hidden, out_act)   # y = the oracle's own output, as its backward read it
    assert R.judge_interval(out, b['out']) == 0
    r_w, over_w = R.judge(dW, b['dW_ref'], b['dW'])
    r_i, over_i = R.judge(d_in, b['d_in_ref'], b['d_in'])
    print(f'oracle, n_hidden {n_hidden}, out_act {out_act}: worst error / budget dW {r_w:.3f}, d_in {r_i:.3f}')
    assert over_w == 0 and over_i == 0, (over_w, over_i, r_w, r_i)
    assert np.count_nonzero(b['dW'] == 0) < 0.2 * b['dW'].size      # (dead rows and nothing else have a zero budget)
    # and the budget is a per-element one: for the median element it is far inside what the tensor-max tolerance of tests/test_gpu_tcnn_parity.py allows
    loose = 2e-2 * np.abs(b['dW_ref']) + 2e-3 * np.abs(b['dW_ref']).max()
    print(f'    median budget / (rtol 2e-2 + atol 2e-3 max|dW|): {np.median(b["dW"] / loose):.3g}')
    assert np.median(b['dW'] / loose) < 1.0


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_every_mutation_of_the_restatement_is_noticed(mut):
    """exact case: `==` fails; random case: some element leaves its budget"""
    c = R.exact_case(129, 2, 0, with_old=True)
    dW, d_in = R.backward(c['fw'], c['W'], c['g'], c['y'], c['loss_scale'], 2, 0, old=c['old'], mut=mut)
    assert not (np.array_equal(dW, c['dW']) and np.array_equal(d_in, c['d_in'])), mut
    r = R.random_case(1025, 2, 1)
    fw = R.forward(r['X'], r['W'], 2, 1)
    b = R.budget(r['X'], r['W'], r['g'], fw['out'], r['loss_scale'], 2, 1, old=r['old'])
    dW, d_in = R.backward(fw, r['W'], r['g'], fw['out'], r['loss_scale'], 2, 1, old=r['old'], mut=mut)
    (r_w, over_w), (r_i, over_i) = R.judge(dW, b['dW_ref'], b['dW']), R.judge(d_in, b['d_in_ref'], b['d_in'])
    print(f'{mut}: {over_w} weight gradients and {over_i} input gradients over budget, worst {max(r_w, r_i):.3g} x')
    assert over_w + over_i > 0, mut
    # unmutated: inside (trivially, it IS the reference) -- the budget call and the backward call agree
    dW, d_in = R.backward(fw, r['W'], r['g'], fw['out'], r['loss_scale'], 2, 1, old=r['old'])
    assert np.array_equal(dW, b['dW_ref']) and np.array_equal(d_in, b['d_in_ref'])


def test_every_generator_of_the_gpu_file_is_provably_exact():
    worst = 0.0
    for kw in R.gpu_exact_cases():
        c = R.exact_case(**kw)
        ok, fp16_max, acc_max = c['exact'], c['fp16_max'], c['acc_max']   # R.exact's verdict on the case, kept by the generator (which asserts it too)
        print(f'{kw}: largest fp16-converted magnitude {fp16_max:g} (limit 2048), worst accumulator {acc_max:.3f} of its limit')
        assert ok and fp16_max <= 2048 and acc_max < 1.0, kw
        worst = max(worst, acc_max)
    for m, nh in R.SIGNED_ZERO_CASES:
        case, twin = R.signed_zero_case(m, nh)
        print(f'signed zero, m {m}, n_hidden {nh}: twin fp16 {twin["fp16_max"]:g}, accumulator {twin["acc_max"]:.3f}')
        assert twin['acc_max'] < 1.0
        # both units dead in the restatement
        assert not case['dW'][:R.W0_N].reshape(64, 32)[[R.SZ_A, R.SZ_B]].any()
    print(f'worst accumulator margin of all generators: {worst:.3f}')


def test_exact_refuses_inexact_inputs():
    c = R.random_case(33, 1, 0)
    assert not R.exact(c['X'], c['W'], c['g'], None, 128.0, 1, 0)[0]
    e = R.exact_case(33, 1, 0)
    assert not R.exact(e['X'], e['W'], e['g'], None, 100.0, 1, 0)[0]           # loss scale not a power of two
    big = e['X'] * 4096.0                                                      # pre-activations beyond fp16's integers
    assert not R.exact(big, e['W'], e['g'], None, 128.0, 1, 0)[0]
