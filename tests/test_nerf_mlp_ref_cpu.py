"""CPU: the float64 restatement of the fused NeRF block (tests/nerf_mlp_ref.py) is the network of nerf.NeRFBlock, its stage budget holds for an f32
device with any summation order, its exact cases are exact, and each planted defect is caught both ways.  Group 17's entry points validate their
arguments on a machine without a GPU, and `render_rays(fused=True)` on CPU tensors is `fused=False`."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nerf_mlp_ref as R
from nerficg_amd import _lib, nerf


def _random_block(width, append, skips, n_color, seed=0, scale=1.0, n_layers=8, k_pos=10, k_dir=4):
    torch.manual_seed(seed)
    block = nerf.NeRFBlock(n_layers, n_color, width, k_pos, k_dir, append, skips)
    if scale != 1.0:
        with torch.no_grad():
            for p in block.parameters():
                p.mul_(scale)
    return block


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('append', [True, False])
@pytest.mark.parametrize('skips', [(), (5,), (2, 5)])
@pytest.mark.parametrize('n_color', [1, 2])
def test_restatement_without_rounding_is_the_double_module(width, append, skips, n_color):
    block = _random_block(width, append, skips, n_color).double()
    net = R.net_from_block(block)
    pos, dirs = R.random_inputs(37, seed=1)
    fw = R.forward(net, pos, dirs, rounding=False)
    with torch.no_grad():
        sigma, rgb = block(torch.from_numpy(pos).double(), torch.from_numpy(dirs).double())
    assert np.abs(fw['sigma'] - sigma.numpy()[:, 0]).max() <= 1e-12
    assert np.abs(fw['rgb'] - rgb.numpy()).max() <= 1e-12


def test_the_module_accepts_zero_frequencies():
    """K = 0 with append_input: the encoding is the identity (what the exact cases rely on)."""
    enc = nerf.FrequencyEncoding(0, True)
    x = torch.randn(5, 3)
    assert enc.get_n_outputs(3) == 3 and torch.equal(enc(x), x)
    block = R.block_from_net(R.exact_net(128, 'identity'))
    pos, dirs = R.exact_inputs(9, 'identity')
    with torch.no_grad():
        sigma, rgb = block(torch.from_numpy(pos), torch.from_numpy(dirs))
    fw = R.forward(R.exact_net(128, 'identity'), pos, dirs)
    assert np.array_equal(sigma.numpy()[:, 0].astype(np.float64), fw['sigma'])     # an exact case is exact for f32 torch as well


def test_the_kernels_sincos_sequence_meets_e_enc():
    """|x| <= 8, k <= 9: a dense random scan, the neighbourhood of 0 and both f32 neighbours of every multiple of pi/2 up to 4096."""
    rng = np.random.default_rng(0)
    args = [(rng.uniform(-8, 8, 400000).astype(np.float32) * np.float32(2.0 ** k)).astype(np.float32) for k in range(10)]
    near = (np.arange(-2607, 2608) * (np.pi / 2)).astype(np.float32)
    args += [np.linspace(-1, 1, 200001).astype(np.float32), near, np.nextafter(near, np.float32(1e9)), np.nextafter(near, np.float32(-1e9))]
    a = np.concatenate(args)
    sn, cs = R.sincos_model(a)
    worst = max(np.abs(sn - np.sin(a.astype(np.float64))).max(), np.abs(cs - np.cos(a.astype(np.float64))).max())
    print(f'worst |f32 sequence - f64| = {worst:.3e} = {worst / R.E_ENC:.3f} E_ENC')
    assert worst <= R.E_ENC
    assert np.array_equal(R.sincos_model(np.zeros(3, np.float32))[0], np.zeros(3)) and np.array_equal(R.sincos_model(np.zeros(3, np.float32))[1], np.ones(3))


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('scale', [1.0, 8.0])
def test_f32_emulation_in_shuffled_order_stays_inside_the_stage_budget(width, scale):
    net = R.net_from_block(_random_block(width, True, (5,), 2, seed=3, scale=scale))
    pos, dirs = R.random_inputs(48, seed=2)
    fw = R.forward(net, pos, dirs)
    rng = np.random.default_rng(5)
    worst = 0.0
    for name in ['H_1', 'H_3', 'H_6', 'sigma', 'F', 'C_1', 'C_2', 'rgb']:
        got = R.f32_stage_shuffled(net, name, fw, rng)
        ref, bound = R.stage_budget(net, name, fw)
        if name == 'rgb':
            assert R.judge_interval(got, bound) == 0, name
            continue
        ratio, over = R.judge(got, ref, bound)
        worst = max(worst, ratio)
        assert over == 0, (name, ratio)
    print(f'W={width} scale={scale}: worst |f32 shuffled - restated| / budget = {worst:.3f}')


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('family', ['identity', 'zero'])
@pytest.mark.parametrize('m', [1, 65, 273])
def test_exact_cases_are_exact(width, family, m):
    net = R.exact_net(width, family)
    pos, dirs = R.exact_inputs(m, family)
    fw = R.forward(net, pos, dirs)
    ok, fp16_max, acc_max = R.exact(net, pos, dirs, fw)
    assert ok and fp16_max <= 2048 and acc_max < 1.0, (ok, fp16_max, acc_max)
    live = {n: int(np.count_nonzero(fw[n])) for n, _ in R.STAGES(net)}
    assert all(v > 0 for v in live.values()), live          # every stage carries non-zero values
    assert R.exact_check(fw, fw) == []


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_planted_defects_break_equality_and_exceed_a_stage_budget(width, mut):
    broken = []
    for family in ('identity', 'zero'):
        net = R.exact_net(width, family)
        pos, dirs = R.exact_inputs(273, family)
        broken += R.exact_check(R.forward(net, pos, dirs), R.forward(net, pos, dirs, mut=mut))
    assert broken, f'{mut}: no exact case notices'
    net = R.net_from_block(_random_block(width, True, (5,), 2, seed=4))
    pos, dirs = R.random_inputs(273, seed=3)
    res = R.chained_check(net, pos, dirs, R.forward(net, pos, dirs, mut=mut))
    assert any(over > 0 for over, _ in res.values()), f'{mut}: inside every stage budget'
    clean = R.chained_check(net, pos, dirs, R.forward(net, pos, dirs))
    assert all(over == 0 for over, _ in clean.values()), clean


def test_group_17_validates_before_it_launches():
    """Null pointers, bad sizes and unsupported shapes are answered before any HIP call (this machine has no GPU)."""
    lib = _lib.load()
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 16
    good = (256, 8, 1, 10, 4, 1, 1 << 5)
    assert lib.nrc_nerf_supported(*good) == 1 and lib.nrc_nerf_supported(128, 1, 3, 0, 0, 1, 0) == 1
    for bad in [(96, 8, 1, 10, 4, 1, 32), (512, 8, 1, 10, 4, 1, 32), (256, 9, 1, 10, 4, 1, 32), (256, 8, 4, 10, 4, 1, 32), (256, 8, 1, 11, 4, 1, 32),
                (256, 8, 1, 10, 5, 1, 32), (256, 8, 1, 0, 4, 0, 32), (256, 8, 1, 10, 4, 1, 1 << 8), (256, 8, 1, 10, 4, 1, 1), (256, 0, 1, 10, 4, 1, 0)]:
        assert lib.nrc_nerf_supported(*bad) == 0, bad
        assert lib.nrc_nerf_packed_bytes(*bad) == -3
        assert lib.nrc_nerf_block_forward(None, None, 1, 0, None, *bad, None, None, 0, None, None) == -3
    # 593 408 weights of the default block as fp16 fragments (padded to whole tiles) + f32 biases
    n = lib.nrc_nerf_packed_bytes(*good)
    assert 2 * 593408 <= n <= 2 * 593408 * 1.15 and n % 16 == 0, n
    assert lib.nrc_nerf_tile_rows() in (64, 128, 256)
    assert lib.nrc_nerf_block_forward(None, None, 1, 0, None, *good, None, None, 0, None, None) == 0          # M == 0: nothing to do
    assert lib.nrc_nerf_block_forward(None, None, 1, 5, None, *good, None, None, 0, None, None) == -1
    assert lib.nrc_nerf_block_forward(None, None, 1, -1, None, *good, None, None, 0, None, None) == -1
    assert lib.nrc_nerf_block_forward(None, None, 0, 0, None, *good, None, None, 0, None, None) == -1          # dir_group < 1
    assert lib.nrc_nerf_block_forward(None, None, 1, 0, None, *good, None, None, 13, None, None) == -1         # 12 stages
    assert lib.nrc_nerf_pack_weights(None, 22, *good, None, None) == -1
    ptrs = (ctypes.c_void_p * 22)(*([16] * 22))
    assert lib.nrc_nerf_pack_weights(ctypes.cast(ptrs, ctypes.c_void_p), 20, *good, ctypes.c_void_p(16), None) == -1   # 11 linears = 22 tensors


def test_fused_config_of_a_block():
    assert nerf.fused_config(nerf.NeRFBlock()) == (256, 8, 1, 10, 4, 1, 1 << 5)
    assert nerf.fused_config(nerf.NeRFBlock(4, 2, 128, 6, 2, False, (1, 3, 9))) == (128, 4, 2, 6, 2, 0, 0b1010)
    assert nerf.fused_config(nerf.NeRFBlock(n_features=96)) is None
    assert nerf.fused_config(nerf.NeRFBlock().double()) is None
    names = nerf.fused_tap_names(nerf.fused_config(nerf.NeRFBlock()))
    assert [n for n, _ in names] == [n for n, _ in R.STAGES(R.net_from_block(nerf.NeRFBlock()))] and names[0][1] == 63 and names[1][1] == 27


@pytest.mark.parametrize('noise', [0.0, 0.5])
def test_render_rays_fused_on_cpu_tensors_is_the_torch_path(noise):
    torch.manual_seed(0)
    coarse, fine = nerf.NeRFBlock(3, 1, 128), nerf.NeRFBlock(3, 1, 128)
    o, d = torch.randn(21, 3), torch.randn(21, 3)
    vd = d / d.norm(dim=-1, keepdim=True)
    out = []
    for fused in (False, True):
        torch.manual_seed(1)
        with torch.no_grad():
            out.append(nerf.render_rays(coarse, fine, o, d, vd, 2.0, 6.0, torch.ones(3), ray_batch_size=8, n_samples_coarse_nerf=8, n_samples_nerf=12,
                                        randomize_samples=True, random_noise_density=noise, fused=fused))
    assert out[0].keys() == out[1].keys()
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    sigma, rgb = nerf.fused_forward(fine, o, vd[:3], dir_group=8)      # 21 samples, 3 direction rows
    ref = fine(o, vd[:3, None, :].expand(-1, 8, -1).reshape(-1, 3)[:21])
    assert torch.equal(sigma, ref[0]) and torch.equal(rgb, ref[1])
