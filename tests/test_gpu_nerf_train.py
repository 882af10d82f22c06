"""GPU: the fused NeRF block's training path (csrc/nerf_net.hip k_nerf_forward<W, 2>, csrc/nerf_grad.hip, nerf.fused_apply, header group 18) against
tests/nerf_grad_ref.py -- the training forward bit for bit against the inference kernel and its taps; every gradient stage, dW and db bit for bit on
provably exact cases; inside per-element budgets taken from the DEVICE's own previous stage on random weights; plus determinism, row independence,
padding, sentinels, the scale, the sanity gate against torch's f32 autograd, the Python layer (fallbacks, accumulation, render_rays, caches, graph
capture) and a small overfitting run against the torch path.

Measured on the MI355X when this file was written: see LABBOOK R21."""
import functools

import numpy as np
import pytest
import torch

from tests import nerf_grad_ref as B
from tests import nerf_mlp_ref as R
from nerficg_amd import _lib, nerf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CHUNK = 2048   # nrc_nerf_wgrad_chunk_rows(); test_chunk_rows_is_what_the_sizes_assume holds the two together
SIZES = [1, 127, 128, 129, 273, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
SHAPES = {'yaml': (8, (5,)), 'one_layer': (1, ()), 'two_skips': (4, (1, 2))}
PAD = 256      # sentinel bytes / elements around the buffers


def test_chunk_rows_is_what_the_sizes_assume():
    assert _lib.load().nrc_nerf_wgrad_chunk_rows() == CHUNK


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def device_run(block, pos, dirs, d_sigma, d_rgb, dir_group=1, grad_scale=0.0, sigma_in=None, rgb_in=None):
    """The C ABI directly: training forward, every saved stage, backward, every gradient stage, grad_params and stats -- as numpy; sentinels around the
    workspace and grad_params are checked on the way."""
    lib, cfg, m = _lib.load(), nerf.fused_config(block), pos.shape[0]
    net = R.net_from_block(block)
    with torch.no_grad():
        blob, blob_t = nerf._train_blobs(block, cfg, torch.device(DEV))
    n_ws, n_grad = lib.nrc_nerf_train_workspace_bytes(*cfg, m), lib.nrc_nerf_grad_params_floats(*cfg)
    ws_all = torch.full((n_ws + 2 * PAD,), 0x5a, dtype=torch.uint8, device=DEV)
    ws = ws_all[PAD:PAD + n_ws]
    p, d = _dev(pos), _dev(dirs)
    sigma, rgb = torch.empty(m, device=DEV), torch.empty(m, 3, device=DEV)
    stream = _lib.stream_of(p)
    _lib.check(lib.nrc_nerf_block_forward_train(_lib.ptr(p), _lib.ptr(d), dir_group, m, _lib.ptr(blob), *cfg, _lib.ptr(sigma), _lib.ptr(rgb), _lib.ptr(ws), stream), 'forward_train')
    out = {'sigma': sigma.cpu().numpy(), 'rgb': rgb.cpu().numpy(), 'taps': {}, 'G': {}}
    for t, (name, width) in enumerate(nerf.fused_tap_names(cfg)):
        buf = torch.empty(m, width, dtype=torch.float16, device=DEV)
        _lib.check(lib.nrc_nerf_saved_stage(_lib.ptr(ws), *cfg, m, t, _lib.ptr(buf), stream), 'saved_stage')
        out['taps'][name] = buf.cpu().numpy().astype(np.float64)
    s_in = sigma if sigma_in is None else _dev(sigma_in)
    r_in = rgb if rgb_in is None else _dev(rgb_in)
    grad_all = torch.full((n_grad + 2 * PAD,), -7.0, device=DEV)
    grad = grad_all[PAD:PAD + n_grad]
    stats = torch.full((4 + 2 * PAD,), -7, dtype=torch.int32, device=DEV)
    ds, dr = _dev(d_sigma), _dev(d_rgb)
    _lib.check(lib.nrc_nerf_block_backward(_lib.ptr(ds), _lib.ptr(dr), _lib.ptr(s_in), _lib.ptr(r_in), m, _lib.ptr(blob_t), *cfg, _lib.ptr(ws), float(grad_scale),
                                           _lib.ptr(grad), _lib.ptr(stats[PAD:]), stream), 'backward')
    for g, name in enumerate(B.BACKWARD_ORDER(net)):
        width = {'rgb': 3, 'sigma': 1, 'C_1': cfg[0] // 2}.get(name, cfg[0])
        buf = torch.empty(m, width, dtype=torch.float16, device=DEV)
        _lib.check(lib.nrc_nerf_grad_stage(_lib.ptr(ws), *cfg, m, g, _lib.ptr(buf), stream), 'grad_stage')
        out['G'][name] = buf.cpu().numpy().astype(np.float64)
    assert bool((ws_all[:PAD] == 0x5a).all()) and bool((ws_all[PAD + n_ws:] == 0x5a).all()), 'workspace sentinels'
    assert bool((grad_all[:PAD] == -7.0).all()) and bool((grad_all[PAD + n_grad:] == -7.0).all()), 'grad_params sentinels'
    assert bool((stats[:PAD] == -7).all()) and bool((stats[PAD + 4:] == -7).all()), 'stats sentinels'
    g = grad.cpu().numpy().astype(np.float64)
    out['grad'], out['stats'], out['dW'], out['db'], at = g, stats[PAD:PAD + 4].cpu().numpy(), [], [], 0
    for w, b in net['lin']:
        out['dW'].append(g[at:at + w.size].reshape(w.shape)); at += w.size
        out['db'].append(g[at:at + b.size]); at += b.size
    assert at == n_grad
    return out


@functools.lru_cache(maxsize=None)
def _exact_block(width, shape, k_pos=0):
    n_layers, skips = SHAPES[shape]
    return R.block_from_net(B.exact_net(width, n_layers, skips, k_pos, 4 if k_pos else 0), DEV)


@functools.lru_cache(maxsize=None)
def _random_block(width, shape, scale=1.0, seed=4):
    """default initialisation times `scale`, the density bias centred on the inputs of R.random_inputs(273, seed=6)"""
    n_layers, skips = SHAPES[shape]
    torch.manual_seed(seed)
    block = nerf.NeRFBlock(n_layers, 1, width, 10, 4, True, skips)
    with torch.no_grad():
        for p in block.parameters():
            p.mul_(scale)
    net = B.centre_density(R.net_from_block(block), *R.random_inputs(273, seed=6))
    return R.block_from_net(net, DEV)


def _exact_cases():
    cases = [(w, 'yaml', 0, m) for w in (128, 256) for m in SIZES]
    cases += [(w, s, 0, m) for w in (128, 256) for s in ('one_layer', 'two_skips') for m in (129, CHUNK + 1)]
    return cases + [(w, 'yaml', 10, 273) for w in (128, 256)]


@pytest.mark.parametrize('width,shape,k_pos,m', _exact_cases())
def test_exact_cases_bit_for_bit(width, shape, k_pos, m):
    block = _exact_block(width, shape, k_pos)
    net = R.net_from_block(block)
    pos, dirs = R.exact_inputs(m, 'identity' if k_pos == 0 else 'zero')
    fw = R.forward(net, pos, dirs)
    d_sigma, d_rgb, sigma, rgb = B.exact_upstream(m)
    bw = B.backward(net, fw, sigma, rgb, d_sigma, d_rgb, 4.0)
    assert R.exact(net, pos, dirs, fw)[0] and B.exact(net, fw, sigma, rgb, d_sigma, d_rgb, 4.0, bw=bw)[0]
    got = device_run(block, pos, dirs, d_sigma, d_rgb, grad_scale=4.0, sigma_in=sigma, rgb_in=rgb)
    assert [n for n in got['taps'] if not np.array_equal(got['taps'][n], fw[n])] == []
    assert B.exact_check(bw, got) == []
    assert list(got['stats']) == [2, 0, 0, 0]


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('m', [1, 129, CHUNK + 1])
def test_training_forward_is_the_inference_forward(width, shape, m):
    """sigma / rgb of fused_apply and of the C entry point equal fused_forward's bit for bit, every saved stage equals the tap of the same stage"""
    block = _random_block(width, shape)
    pos, dirs = R.random_inputs(m, seed=6)
    p, d = _dev(pos), _dev(dirs)
    with torch.no_grad():
        sigma, rgb = nerf.fused_forward(block, p, d)
        taps = {name: nerf.fused_forward(block, p, d, tap=t)[2].cpu().numpy().astype(np.float64)
                for t, (name, _) in enumerate(nerf.fused_tap_names(nerf.fused_config(block)), start=1)}
    s2, r2 = nerf.fused_apply(block, p, d)
    assert s2.requires_grad and r2.requires_grad and torch.equal(s2.detach(), sigma) and torch.equal(r2.detach(), rgb)
    got = device_run(block, pos, dirs, np.zeros(m, np.float32), np.zeros((m, 3), np.float32))
    assert np.array_equal(got['sigma'], sigma[:, 0].cpu().numpy()) and np.array_equal(got['rgb'], rgb.cpu().numpy())
    assert [n for n in taps if not np.array_equal(got['taps'][n], taps[n])] == []


def _budget_case(block, m, seed=6, up_scale=1.0, grad_scale=0.0):
    net = R.net_from_block(block)
    pos, dirs = R.random_inputs(m, seed=seed)
    d_sigma, d_rgb = B.random_upstream(m, seed=seed, scale=up_scale)
    got = device_run(block, pos, dirs, d_sigma, d_rgb, grad_scale=grad_scale)
    S = 2.0 ** int(got['stats'][0])
    res = B.chained_check(net, got['taps'], got['sigma'], got['rgb'], d_sigma, d_rgb, S, got)
    return net, got, res, (pos, dirs, d_sigma, d_rgb, S)


def _worst(res):
    kinds = {}
    for k, (_, r) in res.items():
        kind = k.split('[')[0] + ('[head]' if k in ('G[rgb]', 'G[sigma]') else '')
        kinds[kind] = max(kinds.get(kind, 0.0), r)
    return ' '.join(f'{k}={v:.3f}' for k, v in sorted(kinds.items()))


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('scale', [1.0, 8.0])
@pytest.mark.parametrize('m', SIZES)
def test_chained_budget_on_random_weights(width, scale, m):
    net, got, res, _ = _budget_case(_random_block(width, 'yaml', scale), m)
    assert np.isfinite(got['grad']).all() and (m < 127 or (got['sigma'] > 0).any())
    print(f'W={width} scale={scale} M={m} e={got["stats"][0]} saturated={got["stats"][1]}: {_worst(res)}')
    assert not {k: v for k, v in res.items() if v[0]}
    assert m < 127 or any(np.count_nonzero(g) for g in got['dW'])       # (a single row may have sigma = 0 and a saturated sigmoid)


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('shape', ['one_layer', 'two_skips'])
def test_chained_budget_on_the_other_shapes(width, shape):
    net, got, res, _ = _budget_case(_random_block(width, shape), 273)
    assert not {k: v for k, v in res.items() if v[0]}


@pytest.mark.parametrize('width', [128, 256])
def test_two_calls_give_the_same_bits(width):
    block = _random_block(width, 'yaml')
    pos, dirs = R.random_inputs(CHUNK + 1, seed=6)
    d_sigma, d_rgb = B.random_upstream(CHUNK + 1, seed=6)
    a, b = device_run(block, pos, dirs, d_sigma, d_rgb), device_run(block, pos, dirs, d_sigma, d_rgb)
    assert np.array_equal(a['grad'], b['grad']) and np.array_equal(a['stats'], b['stats'])
    assert all(np.array_equal(a['G'][k], b['G'][k]) for k in a['G'])


@pytest.mark.parametrize('width', [128, 256])
def test_a_rows_gradient_does_not_depend_on_the_batch_or_the_direction_grouping(width):
    block = _random_block(width, 'yaml')
    pos, dirs = R.random_inputs(273, seed=6)
    d_sigma, d_rgb = B.random_upstream(273, seed=6)
    whole = device_run(block, pos, dirs, d_sigma, d_rgb, grad_scale=2.0 ** 14)
    for row in (0, 131, 272):
        one = device_run(block, pos[row:row + 1], dirs[row:row + 1], d_sigma[row:row + 1], d_rgb[row:row + 1], grad_scale=2.0 ** 14)
        assert all(np.array_equal(one['G'][k][0], whole['G'][k][row]) for k in whole['G']), row
    rays = dirs[:5]                                                # 5 rays x 64 samples, the last one cut short
    grouped = device_run(block, pos, rays, d_sigma, d_rgb, dir_group=64, grad_scale=2.0 ** 14)
    expanded = device_run(block, pos, np.repeat(rays, 64, axis=0)[:273], d_sigma, d_rgb, grad_scale=2.0 ** 14)
    assert all(np.array_equal(grouped['G'][k], expanded['G'][k]) for k in grouped['G']) and np.array_equal(grouped['grad'], expanded['grad'])


@pytest.mark.parametrize('width', [128, 256])
def test_a_partial_tile_adds_its_own_rows_only(width):
    """dW of 129 rows = dW of rows 0..127 + dW of row 128, each within its budget (the padded rows of the second workgroup add exactly nothing)"""
    block = _random_block(width, 'yaml')
    net = R.net_from_block(block)
    pos, dirs = R.random_inputs(129, seed=6)
    d_sigma, d_rgb = B.random_upstream(129, seed=6)
    S = 2.0 ** 14
    whole = device_run(block, pos, dirs, d_sigma, d_rgb, grad_scale=S)
    head = device_run(block, pos[:128], dirs[:128], d_sigma[:128], d_rgb[:128], grad_scale=S)
    tail = device_run(block, pos[128:], dirs[128:], d_sigma[128:], d_rgb[128:], grad_scale=S)
    for li in range(len(net['lin'])):
        (_, bw_), (_, bb) = B.weight_budget(net, li, whole['G'], whole['taps'], S)
        (_, hw), (_, hb) = B.weight_budget(net, li, head['G'], head['taps'], S)
        (_, tw), (_, tb) = B.weight_budget(net, li, tail['G'], tail['taps'], S)
        ulp = np.abs(whole['dW'][li]) * 2.0 ** -23            # the sum of the two parts is one more f32 addition
        assert np.all(np.abs(whole['dW'][li] - (head['dW'][li] + tail['dW'][li])) <= bw_ + hw + tw + ulp), li
        assert np.all(np.abs(whole['db'][li] - (head['db'][li] + tail['db'][li])) <= bb + hb + tb + np.abs(whole['db'][li]) * 2.0 ** -23), li
    assert np.array_equal(whole['G']['H_1'][128], tail['G']['H_1'][0])


def test_an_empty_call_launches_nothing_and_bad_arguments_are_refused():
    block = _random_block(128, 'yaml')
    lib, cfg = _lib.load(), nerf.fused_config(block)
    x = torch.zeros(1024, device=DEV)
    with _lib.stage_timer() as timer:
        assert lib.nrc_nerf_block_forward_train(None, None, 1, 0, None, *cfg, None, None, None, _lib.stream_of(x)) == 0
        assert lib.nrc_nerf_block_backward(None, None, None, None, 0, None, *cfg, None, 0.0, None, None, _lib.stream_of(x)) == 0
    assert len(timer.stages) == 0
    assert lib.nrc_nerf_block_backward(None, None, None, None, -1, None, *cfg, None, 0.0, None, None, None) == -1
    assert lib.nrc_nerf_block_backward(None, None, None, None, 5, None, *cfg, None, 0.0, None, None, None) == -1
    assert lib.nrc_nerf_block_backward(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 5, _lib.ptr(x), *cfg, _lib.ptr(x), 3.0, _lib.ptr(x), _lib.ptr(x), None) == -1
    bad = (128, 8, 2, 10, 4, 1, 32)
    assert lib.nrc_nerf_supported(*bad) == 1 and lib.nrc_nerf_train_supported(*bad) == 0
    assert lib.nrc_nerf_train_workspace_bytes(*bad, 5) == -3 and lib.nrc_nerf_train_workspace_bytes(*cfg, -1) == -1


@pytest.mark.parametrize('width', [128, 256])
def test_the_automatic_scale_and_its_exactness(width):
    block = _random_block(width, 'yaml')
    m = 273
    pos, dirs = R.random_inputs(m, seed=6)
    d_sigma, d_rgb = B.random_upstream(m, seed=6)
    a = device_run(block, pos, dirs, d_sigma, d_rgb)
    sigma, rgb = torch.from_numpy(a['sigma']), torch.from_numpy(a['rgb'])
    heads = torch.cat([(torch.from_numpy(d_rgb) * (rgb * (1.0 - rgb))).abs().flatten(), (torch.from_numpy(d_sigma) * (sigma > 0)).abs()])
    assert int(a['stats'][0]) == 12 - int(np.floor(np.log2(float(heads.max())))) and a['stats'][1] == 0
    b = device_run(block, pos, dirs, d_sigma * np.float32(2.0 ** -20), d_rgb * np.float32(2.0 ** -20))
    assert int(b['stats'][0]) == int(a['stats'][0]) + 20
    assert np.array_equal(b['grad'], a['grad'] * 2.0 ** -20) and all(np.array_equal(a['G'][k], b['G'][k]) for k in a['G'])
    # a hand-set scale that overflows fp16: the counter rises, every number stays finite, and the budgets (which know the saturation) still hold
    S = 2.0 ** (int(a['stats'][0]) + 8)
    c = device_run(block, pos, dirs, d_sigma, d_rgb, grad_scale=S)
    assert c['stats'][0] == a['stats'][0] + 8 and c['stats'][1] > 0 and np.isfinite(c['grad']).all()
    net = R.net_from_block(block)
    # elements that certainly overflowed: the heads' f32 values (restated exactly), and every restated |dX| beyond 65520 by more than its f32 error
    sure = sum(int(np.count_nonzero(np.abs(g) >= 65520.0)) for g in B.head_gradients(c['sigma'], c['rgb'], d_sigma, d_rgb, S, raw=True))
    for name in B.BACKWARD_ORDER(net)[1:3] + B.BACKWARD_ORDER(net)[4:]:
        st = B.data_gradient(net, name, c['G'], c['taps'])
        sure += int(np.count_nonzero(st['mask'] & (np.abs(st['Z']) - B.gamma32(st['n_terms'] + 2) * st['abs'] >= 65520.0)))
    at_limit = sum(int(np.count_nonzero(np.abs(g) == 65504.0)) for g in c['G'].values())      # saturated, or rounded to the largest finite number
    assert 0 < sure <= c['stats'][1] <= at_limit
    res = B.chained_check(net, c['taps'], c['sigma'], c['rgb'], d_sigma, d_rgb, S, c)
    assert not {k: v for k, v in res.items() if v[0]}
    z = device_run(block, pos, dirs, np.zeros(m, np.float32), np.full((m, 3), np.nan, np.float32))      # must not fault; numbers unspecified
    assert z['stats'][0] == 0


def _torch_grads(block, pos, dirs, d_sigma, d_rgb):
    block.zero_grad(set_to_none=True)
    sigma, rgb = block(_dev(pos), _dev(dirs))
    ((sigma[:, 0] * _dev(d_sigma)).sum() + (rgb * _dev(d_rgb)).sum()).backward()
    grads = [(lin.weight.grad.double().cpu().numpy(), lin.bias.grad.double().cpu().numpy()) for lin in nerf._block_linears(block)]
    block.zero_grad(set_to_none=True)
    return grads


@pytest.mark.parametrize('width', [128, 256])
def test_sanity_gate_against_torch_f32_autograd(width):
    """C = max |restatement - torch f32 autograd| per parameter tensor (what fp16 operands and gradients cost by themselves); the device stays within 2 C."""
    block = _random_block(width, 'yaml')
    net = R.net_from_block(block)
    m = CHUNK + 1
    pos, dirs = R.random_inputs(m, seed=12)
    d_sigma, d_rgb = B.random_upstream(m, seed=12)
    got = device_run(block, pos, dirs, d_sigma, d_rgb)
    fw = R.forward(net, pos, dirs)
    ref = B.backward(net, fw, fw['sigma'], fw['rgb'], d_sigma, d_rgb, 2.0 ** int(got['stats'][0]))
    worst = 0.0
    for li, (tw, tb) in enumerate(_torch_grads(block, pos, dirs, d_sigma, d_rgb)):
        for name, t, r, g in (('dW', tw, ref['dW'][li], got['dW'][li]), ('db', tb, ref['db'][li], got['db'][li])):
            c, e = np.abs(r - t).max(), np.abs(g - t).max()
            worst = max(worst, e / c)
            assert e <= 2.0 * c, (name, li, e, c)
    print(f'W={width}: device vs torch f32 relative to C, worst tensor: {worst:.3f}')


# ------------------------------------------------------------------------------------------------ the Python layer
def _rays(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.3
    d = torch.randn(n, 3, generator=g)
    return o.to(DEV), d.to(DEV), (d / d.norm(dim=-1, keepdim=True)).to(DEV)


@pytest.mark.parametrize('case', ['cpu', 'width_96', 'positions_require_grad', 'two_colour_layers'])
def test_ineligible_calls_give_torchs_bits_and_gradients(case):
    torch.manual_seed(3)
    dev = 'cpu' if case == 'cpu' else DEV
    block = nerf.NeRFBlock(3, 2 if case == 'two_colour_layers' else 1, 96 if case == 'width_96' else 128).to(dev)
    pos, dirs = (torch.from_numpy(a).to(dev) for a in R.random_inputs(100, seed=2))
    rays = dirs[:4].contiguous()
    if case == 'positions_require_grad':
        pos.requires_grad_()
    results = []
    for fused in (False, True):
        block.zero_grad(set_to_none=True)
        pos.grad = None
        expanded = rays[:, None, :].expand(-1, 25, -1).reshape(-1, 3)
        sigma, rgb = nerf.fused_apply(block, pos, rays, dir_group=25) if fused else block(pos, expanded)
        (sigma.square().sum() + rgb.square().sum()).backward()
        results.append([sigma.detach(), rgb.detach()] + [p.grad.clone() for p in block.parameters()] + ([pos.grad.clone()] if pos.grad is not None else []))
    assert len(results[0]) == len(results[1]) and all(torch.equal(a, b) for a, b in zip(*results))
    assert 'workspaces' not in block.__dict__.get('_fused_cache', {})                      # the training kernels never ran


def test_gradients_accumulate_and_the_caches_follow_an_optimizer_step():
    torch.manual_seed(2)
    block = nerf.NeRFBlock(4, 1, 128).to(DEV)
    pos, dirs = (torch.from_numpy(a).to(DEV) for a in R.random_inputs(200, seed=3))
    w = torch.linspace(0.5, 1.5, 200, device=DEV)[:, None]

    def step():
        sigma, rgb = nerf.fused_apply(block, pos, dirs)
        ((sigma * w).sum() + (rgb * w).sum()).backward()
    step()
    once = [p.grad.clone() for p in block.parameters()]
    assert all(bool(torch.isfinite(g).all()) for g in once) and sum(float(g.abs().sum()) for g in once) > 0
    stats = nerf.fused_grad_stats(block)
    assert stats.dtype == torch.int32 and stats.is_cuda and int(stats[1]) == 0
    step()
    assert all(torch.equal(p.grad, g + g) for p, g in zip(block.parameters(), once))          # the same bits twice: x + x is exact
    cache = block._fused_cache
    assert cache['packs'] == 1 and cache['packs_t'] == 1 and len(cache['workspaces']) == 1   # nothing repacked, one workspace reused
    torch.optim.SGD(block.parameters(), lr=0.05).step()
    block.zero_grad(set_to_none=True)
    with _lib.stage_timer() as timer:
        step()
    assert cache['packs'] == 2 and cache['packs_t'] == 2
    assert [n for n, _ in timer.stages] == ['k_nerf_pack', 'k_nerf_pack_t', 'k_nerf_forward_train', 'k_nerf_head_max', 'k_nerf_dgrad', 'k_nerf_wgrad', 'k_nerf_wreduce']
    assert not any(torch.equal(p.grad, g) for p, g in zip(block.parameters(), once))
    with torch.no_grad():                                                                      # under no_grad: the inference kernel
        with _lib.stage_timer() as timer:
            nerf.fused_apply(block, pos, dirs)
    assert [n for n, _ in timer.stages] == ['k_nerf_forward']


def test_render_rays_wiring_adds_nothing():
    """render_rays(fused_train=True) equals the torch pipeline run on the device's own fused_apply values, gradients included."""
    torch.manual_seed(5)
    coarse, fine = nerf.NeRFBlock(4, 1, 128).to(DEV), nerf.NeRFBlock(8, 1, 256).to(DEV)
    o, d, vd = _rays(64, seed=1)
    bg = torch.tensor([1.0, 0.5, 0.25])

    class Through(torch.nn.Module):           # a module with the torch calling convention that answers with the fused training path's values
        def __init__(self, block):
            super().__init__()
            self.block = block

        def forward(self, positions, directions, noise=0.0):
            return nerf.fused_apply(self.block, positions.contiguous(), directions.contiguous())
    results = []
    for through in (False, True):
        for b in (coarse, fine):
            b.zero_grad(set_to_none=True)
        c, f = (Through(coarse), Through(fine)) if through else (coarse, fine)
        out = nerf.render_rays(c, f, o, d, vd, 2.0, 6.0, bg, ray_batch_size=48, n_samples_coarse_nerf=16, n_samples_nerf=48, fused_train=not through)
        (out['rgb'].square().mean() + out['rgb_coarse'].square().mean()).backward()
        results.append(({k: v.detach().clone() for k, v in out.items()}, [p.grad.clone() for b in (coarse, fine) for p in b.parameters()]))
    for k in results[0][0]:
        assert torch.equal(results[0][0][k], results[1][0][k]), k
    assert all(torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))
    assert sum(float(g.abs().sum()) for g in results[0][1]) > 0
    assert len(fine._fused_cache['workspaces']) == 2               # two ray chunks in flight before the backward: two workspaces


def test_forward_backward_and_adam_capture_into_one_graph():
    def fresh():
        torch.manual_seed(8)
        block = nerf.NeRFBlock(4, 1, 128).to(DEV)
        return block, torch.optim.Adam(block.parameters(), lr=5e-4, capturable=True)
    pos, dirs = (torch.from_numpy(a).to(DEV) for a in R.random_inputs(300, seed=4))
    target = torch.rand(300, 3, generator=torch.Generator().manual_seed(1)).to(DEV)

    def step(block, opt):
        opt.zero_grad(set_to_none=True)
        sigma, rgb = nerf.fused_apply(block, pos, dirs)
        loss = (rgb - target).square().mean() + sigma.mean() * 1e-3
        loss.backward()
        opt.step()
    block, opt = fresh()
    for _ in range(2):                             # the warm-up step and the replayed one
        step(block, opt)
    eager = [p.detach().clone() for p in block.parameters()]
    block, opt = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(block, opt)                            # warm-up on the capture stream: allocations, Adam's state
    torch.cuda.current_stream().wait_stream(side)
    del block.__dict__['_fused_cache']              # the capture records both packs
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(block, opt)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), e) for p, e in zip(block.parameters(), eager))


def _steps_to_half(fused_train, limit):
    """Adam steps until the loss of a small overfitting run is half of its initial value (checked every fifth step), None beyond `limit`.  64 fixed rays
    with fixed target colours (a smooth function of the viewing direction), a 4 x 128 coarse and fine block, the configuration's learning rate 5e-4.
    The density biases start at 0.5: a freshly initialised block has sigma = 0 on nearly all of space, and neither path trains through a closed ReLU."""
    o, d, vd = _rays(64, seed=3)
    target, bg = (0.5 + 0.5 * vd).contiguous(), torch.ones(3)
    torch.manual_seed(21)
    coarse, fine = nerf.NeRFBlock(4, 1, 128).to(DEV), nerf.NeRFBlock(4, 1, 128).to(DEV)
    with torch.no_grad():
        for b in (coarse, fine):
            b.density_layer.bias.fill_(0.5)
    opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)
    first = None
    for it in range(limit + 1):
        opt.zero_grad(set_to_none=True)
        out = nerf.render_rays(coarse, fine, o, d, vd, 2.0, 6.0, bg, n_samples_coarse_nerf=16, n_samples_nerf=32, fused_train=fused_train)
        loss = (out['rgb'] - target).square().mean() + (out['rgb_coarse'] - target).square().mean()
        if it % 5 == 0:                              # one host read every five steps
            value = float(loss.detach())
            first = value if first is None else first
            if value <= 0.5 * first:
                return it
        loss.backward()
        opt.step()
    return None


def test_training_halves_the_loss_about_as_fast_as_torch():
    """The fused path must halve the initial loss within 1.5 x the step count of the torch f32 path on the same data and seed (the margin covers fp16
    operands).  Measured on the MI355X (LABBOOK R21): torch f32 30 steps, fused 30 steps."""
    n_torch = _steps_to_half(False, 1000)
    assert n_torch is not None and n_torch > 0
    n_fused = _steps_to_half(True, int(1.5 * n_torch))
    print(f'steps to half the initial loss: torch f32 {n_torch}, fused {n_fused}')
    assert n_fused is not None and n_fused <= 1.5 * n_torch
