"""CPU: tests/nerf_grad_ref.py checks itself -- its exact cases are exact (also under a shuffled f32 summation), each planted defect of the restatement
breaks equality on an exact case and leaves a budget on a random one, and the plain chain rule of the restatement agrees with torch's float64 autograd
through a straight-through fp16 module.  None of this pins the device: tests/test_gpu_nerf_train.py does."""
import numpy as np
import pytest
import torch

from tests import nerf_grad_ref as B
from tests import nerf_mlp_ref as R


def _exact_case(width, n_layers, skips, k_pos, m, S=4.0):
    net = B.exact_net(width, n_layers, skips, k_pos, 4 if k_pos else 0)
    pos, dirs = R.exact_inputs(m, 'identity' if k_pos == 0 else 'zero')
    fw = R.forward(net, pos, dirs)
    assert R.exact(net, pos, dirs, fw)[0]
    d_sigma, d_rgb, sigma, rgb = B.exact_upstream(m)
    return net, fw, (sigma, rgb, d_sigma, d_rgb, S)


def _random_case(width, n_layers, skips, m, seed=3, S=2.0 ** 14):
    torch.manual_seed(seed)
    from nerficg_amd import nerf
    net = R.net_from_block(nerf.NeRFBlock(n_layers, 1, width, 10, 4, True, skips))
    pos, dirs = R.random_inputs(m, seed=seed)
    net = B.centre_density(net, pos, dirs)
    fw = R.forward(net, pos, dirs)
    assert 0.25 < (fw['sigma'] > 0).mean() < 0.75
    d_sigma, d_rgb = B.random_upstream(m, seed=seed)
    return net, fw, (fw['sigma'].astype(np.float32), fw['rgb'].astype(np.float32), d_sigma, d_rgb, S)


@pytest.mark.parametrize('shape', [(128, 8, (5,), 0), (256, 8, (5,), 0), (128, 1, (), 0), (128, 4, (1, 2), 0), (128, 8, (2, 5), 10)])
@pytest.mark.parametrize('m', [1, 129, 4097])
def test_exact_cases_are_exact(shape, m):
    width, n_layers, skips, k_pos = shape
    net, fw, up = _exact_case(width, n_layers, skips, k_pos, m)
    bw = B.backward(net, fw, *up)
    ok, ratio = B.exact(net, fw, *up, bw=bw)
    assert ok, ratio
    assert any(np.count_nonzero(g) for g in bw['dW']) and np.count_nonzero(bw['G']['H_1'])        # not exact because it is empty


def test_exact_means_any_f32_order_gives_the_same_bits():
    net, fw, up = _exact_case(128, 4, (1, 2), 0, 273)
    bw = B.backward(net, fw, *up)
    rng = np.random.default_rng(5)
    for _ in range(2):
        st = B.data_gradient(net, 'H_2', bw['G'], fw)
        assert np.array_equal(B.shuffled_f32(bw['G']['H_3'], B._w16(net, 2)[:, :128], rng), st['Z'])
        X, gname = B.linear_operand(net, 2, fw)
        assert np.array_equal(B.shuffled_f32(bw['G'][gname].T, X, rng) / up[-1], bw['dW'][2])
        assert np.array_equal(B.shuffled_f32(bw['G'][gname].T, np.ones((273, 1)), rng)[:, 0] / up[-1], bw['db'][2])


@pytest.mark.parametrize('mut', B.MUTATIONS)
def test_each_planted_defect_is_seen(mut):
    net, fw, up = _exact_case(128, 8, (2, 5), 0, 273)
    good, bad = B.backward(net, fw, *up), B.backward(net, fw, *up, mut=mut)
    assert B.exact_check(good, good) == []
    assert B.exact_check(good, bad), f'{mut}: equal on the exact case'
    net, fw, up = _random_case(128, 8, (2, 5), 273)
    res = B.chained_check(net, fw, *up, B.backward(net, fw, *up))
    assert not {k: v for k, v in res.items() if v[0]}
    res = B.chained_check(net, fw, *up, B.backward(net, fw, *up, mut=mut))
    assert {k: v for k, v in res.items() if v[0]}, f'{mut}: inside every budget on the random case'


def test_a_shuffled_f32_device_stays_inside_the_budgets():
    """What any summation order may return: inside the G budget and the dW budget."""
    net, fw, up = _random_case(128, 4, (1, 2), 129)
    bw = B.backward(net, fw, *up)
    rng = np.random.default_rng(7)
    ref, bound = B.stage_budget(net, 'H_2', bw['G'], fw)
    z = B.shuffled_f32(bw['G']['H_3'], B._w16(net, 2)[:, :128], rng)
    got = np.where(fw['H_2'] > 0, B.sat(B.h16(z)), 0.0)
    assert B.judge(got, ref, bound)[1] == 0
    X, gname = B.linear_operand(net, 2, fw)
    (dw, bound), _ = B.weight_budget(net, 2, bw['G'], fw, up[-1])
    ratio, over = B.judge(B.shuffled_f32(bw['G'][gname].T, X, rng) / up[-1], dw, bound)
    assert over == 0 and ratio < 0.5


def test_the_chain_rule_of_the_restatement_is_autograd_through_a_straight_through_fp16_module():
    net, fw, up = _random_case(128, 4, (1, 2), 65, S=1.0)
    sigma, rgb, d_sigma, d_rgb, _ = up
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ste = lambda t: t + (t64(B.sat(B.h16(t.detach().numpy()))) - t.detach())            # value: the fp16 number; gradient: identity
    params = [(t64(w).requires_grad_(), t64(b).requires_grad_()) for w, b in net['lin']]
    lin = lambda k, x: x @ ste(params[k][0]).T + params[k][1]
    L = net['L']
    enc_pos, enc_dir = t64(fw['enc_pos']), t64(fw['enc_dir'])
    h = enc_pos
    for l in range(L):
        x = torch.cat([h, enc_pos], dim=1) if l in net['skips'] else h
        h = torch.relu(ste(lin(l, x)))                                                   # mask: the fp16 operand > 0
        assert np.array_equal(h.detach().numpy(), fw[f'H_{l + 1}'])
    s = torch.relu(lin(L, h))[:, 0]
    f = ste(lin(L + 1, h))
    c = torch.relu(ste(lin(L + 2, torch.cat([f, enc_dir], dim=1))))
    out = torch.sigmoid(lin(L + 3, c))
    ((s * t64(d_sigma)).sum() + (out * t64(d_rgb)).sum()).backward()
    bw = B.backward(net, fw, s.detach().numpy(), out.detach().numpy(), d_sigma, d_rgb, 1.0, rounding=False)
    for k, (w, b) in enumerate(params):
        for got, ref in ((bw['dW'][k], w.grad.numpy()), (bw['db'][k], b.grad.numpy())):
            assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-30), k
