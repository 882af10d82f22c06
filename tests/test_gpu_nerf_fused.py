"""GPU: the fused NeRF block (nerficg_amd/csrc/nerf_net.hip, nerf.fused_forward) against tests/nerf_mlp_ref.py -- bit for bit on provably exact
cases, stage by stage inside the chained budget on random weights (each stage judged from the DEVICE's own previous tap), plus row independence,
sentinels, saturation, the weight cache, the fallbacks, render_rays wiring, the sanity gate against the f32 module and graph capture.

Measured on the MI355X when this file was written (LABBOOK R20): every exact case equal; chained budget worst error / bound 1.00 on the fp16 stages and
the encodings (one fp16 ulp where a rounding boundary lies inside the error interval: the bound's own size), 0.01 on sigma, no element over its bound;
sanity gate, device against the f32 module relative to C: sigma 1.000 / 1.000, rgb 1.001 / 0.946 (W = 128 / 256; gate 2)."""
import functools

import numpy as np
import pytest
import torch

from tests import nerf_mlp_ref as R
from nerficg_amd import _lib, nerf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _tile():
    return _lib.load().nrc_nerf_tile_rows()


def _sizes():
    t = 128   # nrc_nerf_tile_rows(); test_tile_rows_is_what_the_sizes_assume holds the two together
    return [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 17, 4097]


def test_tile_rows_is_what_the_sizes_assume():
    assert _tile() == 128


def device_run(block, pos, dirs, dir_group=1, taps=True):
    """dict of every stage the device can show (one launch per tap) + sigma, rgb, as numpy"""
    p, d = torch.from_numpy(np.ascontiguousarray(pos)).to(DEV), torch.from_numpy(np.ascontiguousarray(dirs)).to(DEV)
    with torch.no_grad():
        sigma, rgb = nerf.fused_forward(block, p, d, dir_group)
        out = {'sigma': sigma[:, 0].cpu().numpy(), 'rgb': rgb.cpu().numpy()}
        if taps:
            for t, (name, width) in enumerate(nerf.fused_tap_names(nerf.fused_config(block)), start=1):
                s2, r2, tapped = nerf.fused_forward(block, p, d, dir_group, tap=t)
                assert tapped.shape == (pos.shape[0], width) and tapped.dtype == torch.float16
                assert torch.equal(s2, sigma) and torch.equal(r2, rgb), f'the tap instantiation ({name}) computes other outputs'
                out[name] = tapped.cpu().numpy().astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def _exact_block(width, family):
    return R.block_from_net(R.exact_net(width, family), DEV)


@functools.lru_cache(maxsize=None)
def _random_block(width, scale, n_color=2, skips=(5,), seed=4):
    torch.manual_seed(seed)
    block = nerf.NeRFBlock(8, n_color, width, 10, 4, True, skips)
    if scale != 1.0:
        with torch.no_grad():
            for p in block.parameters():
                p.mul_(scale)
    return block.to(DEV)


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('family', ['identity', 'zero'])
@pytest.mark.parametrize('m', _sizes())
def test_exact_cases_bit_for_bit(width, family, m):
    net = R.exact_net(width, family)
    pos, dirs = R.exact_inputs(m, family)
    fw = R.forward(net, pos, dirs)
    assert R.exact(net, pos, dirs, fw)[0]
    got = device_run(_exact_block(width, family), pos, dirs)
    assert R.exact_check(fw, got) == []


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('scale', [1.0, 8.0])
@pytest.mark.parametrize('m', _sizes())
def test_chained_budget_on_random_weights(width, scale, m):
    block = _random_block(width, scale)
    net = R.net_from_block(block)
    pos, dirs = R.random_inputs(m, seed=6)
    got = device_run(block, pos, dirs)
    assert all(np.isfinite(v).all() for v in got.values())
    res = R.chained_check(net, pos, dirs, got)
    print(f'W={width} scale={scale} M={m}: ' + ' '.join(f'{k}={r:.2f}' for k, (_, r) in res.items()))
    assert not {k: v for k, v in res.items() if v[0]}


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('cfg', [dict(n_layers=1, n_color=1, k_pos=0, k_dir=0, append=True, skips=()),
                                 dict(n_layers=3, n_color=3, k_pos=10, k_dir=4, append=False, skips=(1, 2)),
                                 dict(n_layers=8, n_color=1, k_pos=10, k_dir=4, append=True, skips=(1, 2, 3, 4, 5, 6, 7)),
                                 dict(n_layers=5, n_color=2, k_pos=4, k_dir=1, append=True, skips=())])
def test_chained_budget_on_other_supported_shapes(width, cfg):
    torch.manual_seed(9)
    block = nerf.NeRFBlock(cfg['n_layers'], cfg['n_color'], width, cfg['k_pos'], cfg['k_dir'], cfg['append'], cfg['skips']).to(DEV)
    assert nerf.fused_config(block) is not None
    pos, dirs = R.random_inputs(273, seed=8)
    res = R.chained_check(R.net_from_block(block), pos, dirs, device_run(block, pos, dirs))
    assert not {k: v for k, v in res.items() if v[0]}


@pytest.mark.parametrize('width', [128, 256])
def test_rows_do_not_depend_on_the_batch_or_the_direction_grouping(width):
    block = _random_block(width, 1.0)
    pos, dirs = R.random_inputs(4097, seed=6)
    whole = device_run(block, pos, dirs, taps=False)
    part = device_run(block, pos[1000:1100], dirs[1000:1100], taps=False)
    for k in ('sigma', 'rgb'):
        assert np.array_equal(whole[k][1000:1100], part[k]), k
    rays = dirs[:65]                                             # 65 rays x 64 samples, the last ray cut short
    grouped = device_run(block, pos[:4097], rays, dir_group=64, taps=False)
    expanded = device_run(block, pos[:4097], np.repeat(rays, 64, axis=0)[:4097], taps=False)
    for k in ('sigma', 'rgb'):
        assert np.array_equal(grouped[k], expanded[k]), k


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('m', [0, 1, 129])
def test_sentinels_survive_and_an_empty_call_launches_nothing(width, m):
    block = _random_block(width, 1.0)
    cfg = nerf.fused_config(block)
    lib = _lib.load()
    nerf.fused_forward(block, torch.zeros(1, 3, device=DEV), torch.zeros(1, 3, device=DEV))      # the blob exists
    blob = block._fused_cache['blob']
    pos, dirs = (torch.from_numpy(a).to(DEV) for a in R.random_inputs(max(m, 1), seed=2))
    pad = 64
    for tap, (name, w) in [(0, ('none', 1))] + list(enumerate(nerf.fused_tap_names(cfg), start=1)):
        sigma = torch.full((m + pad,), -7.0, device=DEV)
        rgb = torch.full((3 * m + pad,), -7.0, device=DEV)
        tapped = torch.full((m * w + pad,), -7.0, dtype=torch.float16, device=DEV)
        with _lib.stage_timer() as timer:
            _lib.check(lib.nrc_nerf_block_forward(_lib.ptr(pos), _lib.ptr(dirs), 1, m, _lib.ptr(blob), *cfg, _lib.ptr(sigma), _lib.ptr(rgb), tap,
                                                  _lib.ptr(tapped), _lib.stream_of(pos)), 'nerf_block_forward')
        assert len(timer.stages) == (1 if m else 0)
        assert bool((sigma[m:] == -7.0).all()) and bool((rgb[3 * m:] == -7.0).all()) and bool((tapped[m * w if tap else 0:] == -7.0).all()), name
        assert bool((sigma[:m] >= 0).all()) and bool((rgb[:3 * m] > 0).all())
        if tap and m:
            assert bool((tapped[:m * w] != -7.0).all()), name


@pytest.mark.parametrize('width', [128, 256])
def test_a_hidden_unit_past_65504_saturates(width):
    base = R.exact_net(width, 'identity')
    lin = [(w.copy(), b.copy()) for w, b in base['lin']]
    lin[0][0][5, :] = 0.0
    lin[0][0][5, 0] = 32768.0           # unit 5 of H_1 = relu(32768 x + b): 98304 for x = 3 -- inf as fp16, 65504 after saturation
    lin[1][0][7, :] = 0.0
    lin[1][0][7, 5] = 1.0               # and one unit of H_2 reads it
    net = R.make_net(lin, base['L'], base['n_color'], base['k_pos'], base['k_dir'], True, base['skips'])
    pos, dirs = R.exact_inputs(65, 'identity')
    pos[3, 0], pos[4, 0] = 3.0, 2.0
    fw = R.forward(net, pos, dirs)
    assert fw['H_1'][3, 5] == 65504.0 and fw['H_1'][4, 5] == 65504.0 and fw['H_2'][3, 7] >= 65504.0
    got = device_run(R.block_from_net(net, DEV), pos, dirs)
    assert all(np.isfinite(v).all() for v in got.values())
    for name in ('H_1', 'H_2', 'H_3'):
        assert np.array_equal(got[name], fw[name]), name
    res = R.chained_check(net, pos, dirs, got)
    assert not {k: v for k, v in res.items() if v[0]}


def test_the_cache_follows_the_parameters():
    torch.manual_seed(2)
    block = nerf.NeRFBlock(4, 1, 128).to(DEV)
    pos, dirs = (torch.from_numpy(a).to(DEV) for a in R.random_inputs(200, seed=3))
    with torch.no_grad():
        a = nerf.fused_forward(block, pos, dirs)
        packs = block._fused_cache['packs']
        with _lib.stage_timer() as timer:
            b = nerf.fused_forward(block, pos, dirs)
        assert block._fused_cache['packs'] == packs == 1 and [n for n, _ in timer.stages] == ['k_nerf_forward']     # unchanged: no repack
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        block.initial_layers[1][0].weight[3, 4] += 0.5                                                                 # in place
        with _lib.stage_timer() as timer:
            c = nerf.fused_forward(block, pos, dirs)
        assert block._fused_cache['packs'] == 2 and [n for n, _ in timer.stages] == ['k_nerf_pack', 'k_nerf_forward']
        assert not torch.equal(a[1], c[1])
    opt = torch.optim.SGD(block.parameters(), lr=0.05)
    sigma, rgb = block(pos, dirs)
    (sigma.sum() + rgb.sum()).backward()
    opt.step()
    with torch.no_grad():
        d = nerf.fused_forward(block, pos, dirs)
    assert block._fused_cache['packs'] == 3 and not torch.equal(c[1], d[1])
    res = R.chained_check(R.net_from_block(block), pos.cpu().numpy(), dirs.cpu().numpy(), device_run(block, pos.cpu().numpy(), dirs.cpu().numpy()))
    assert not {k: v for k, v in res.items() if v[0]}


def _rays(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.3
    d = torch.randn(n, 3, generator=g)
    return o.to(DEV), d.to(DEV), (d / d.norm(dim=-1, keepdim=True)).to(DEV)


@pytest.mark.parametrize('case', ['grad', 'noise', 'width_96'])
def test_fallbacks_give_the_bits_of_the_torch_path(case):
    torch.manual_seed(3)
    width = 96 if case == 'width_96' else 128
    coarse, fine = nerf.NeRFBlock(3, 1, width).to(DEV), nerf.NeRFBlock(3, 1, width).to(DEV)
    o, d, vd = _rays(40)
    results = []
    for fused in (False, True):
        for b in (coarse, fine):
            b.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        with torch.set_grad_enabled(case == 'grad'):
            out = nerf.render_rays(coarse, fine, o, d, vd, 2.0, 6.0, torch.ones(3), ray_batch_size=16, n_samples_coarse_nerf=8, n_samples_nerf=16,
                                   random_noise_density=0.5 if case == 'noise' else 0.0, fused=fused)
            loss = out['rgb'].square().mean() + out['rgb_coarse'].square().mean()
            grads = []
            if case == 'grad':
                loss.backward()
                grads = [p.grad.clone() for b in (coarse, fine) for p in b.parameters()]
        results.append((loss.detach().clone(), {k: v.detach().clone() for k, v in out.items()}, grads))
    assert torch.equal(results[0][0], results[1][0])
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k
    assert len(results[0][2]) == len(results[1][2]) and all(torch.equal(a, b) for a, b in zip(results[0][2], results[1][2]))
    assert '_fused_cache' not in fine.__dict__                      # the kernel never ran


def test_render_rays_wiring_adds_nothing():
    """64 rays x (16 + 48) samples: the fused render equals the torch pipeline run on the device's own fused sigma / rgb."""
    torch.manual_seed(5)
    coarse, fine = nerf.NeRFBlock(4, 1, 128).to(DEV), nerf.NeRFBlock(8, 1, 256).to(DEV)
    o, d, vd = _rays(64, seed=1)
    bg = torch.tensor([1.0, 0.5, 0.25])
    with torch.no_grad():
        out = nerf.render_rays(coarse, fine, o, d, vd, 2.0, 6.0, bg, ray_batch_size=48, n_samples_coarse_nerf=16, n_samples_nerf=48, fused=True)

        class Through(torch.nn.Module):           # a module with the torch calling convention that answers with the fused kernel's values
            def __init__(self, block):
                super().__init__()
                self.block = block

            def forward(self, positions, directions, noise=0.0):
                return nerf.fused_forward(self.block, positions.contiguous(), directions.contiguous())
        ref = nerf.render_rays(Through(coarse), Through(fine), o, d, vd, 2.0, 6.0, bg, ray_batch_size=48, n_samples_coarse_nerf=16, n_samples_nerf=48)
    assert set(out) == {'rgb', 'alpha', 'depth', 'rgb_coarse', 'alpha_coarse', 'depth_coarse'}
    for k in out:
        assert out[k].shape[0] == 64 and bool(torch.isfinite(out[k]).all()), k
        assert torch.equal(out[k], ref[k]), k
    assert coarse._fused_cache['packs'] == 1 and fine._fused_cache['packs'] == 1


@pytest.mark.parametrize('width', [128, 256])
def test_sanity_gate_against_the_f32_module(width):
    """C = max |restatement - torch f32| (what fp16 operands cost by themselves); the device must stay within 2 C of torch f32."""
    torch.manual_seed(7)
    block = nerf.NeRFBlock(8, 1, width).to(DEV)
    pos, dirs = R.random_inputs(4097, seed=12)
    with torch.no_grad():
        ts, tr = block(torch.from_numpy(pos).to(DEV), torch.from_numpy(dirs).to(DEV))
    ts, tr = ts[:, 0].double().cpu().numpy(), tr.double().cpu().numpy()
    fw = R.forward(R.net_from_block(block), pos, dirs)
    got = device_run(block, pos, dirs, taps=False)
    for name, t in (('sigma', ts), ('rgb', tr)):
        c = np.abs(fw[name] - t).max()
        e = np.abs(got[name].astype(np.float64) - t).max()
        print(f'W={width} {name}: C = {c:.3e}, device vs torch f32 = {e:.3e}, ratio = {e / c:.3f}')
        assert e <= 2.0 * c, (name, e, c)


def test_forward_and_pack_capture_into_a_graph():
    torch.manual_seed(8)
    block = nerf.NeRFBlock(8, 1, 256).to(DEV)
    pos, dirs = (torch.from_numpy(a).to(DEV) for a in R.random_inputs(300, seed=4))
    with torch.no_grad():
        eager = nerf.fused_forward(block, pos, dirs)
        del block.__dict__['_fused_cache']           # the capture records the pack as well
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            nerf.fused_forward(block, pos, dirs)     # warm-up on the capture stream
            del block.__dict__['_fused_cache']
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sigma, rgb = nerf.fused_forward(block, pos, dirs)
        assert block._fused_cache['packs'] == 1
        for _ in range(2):
            sigma.fill_(-1.0)
            rgb.fill_(-1.0)
            block._fused_cache['blob'].zero_()        # the replay must repack
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(sigma, eager[0]) and torch.equal(rgb, eager[1])
