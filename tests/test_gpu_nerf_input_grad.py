"""GPU: the vanilla NeRF path's gradients to its inputs (C ABI group 20: csrc/nerf_input_grad.hip, the two ray stages of csrc/nerf_rays.hip, and
input_grad=True on nerf.fused_apply / sample_coarse / sample_fine / composite / render_rays) against tests/nerf_input_grad_ref.py -- every encoded-input
gradient, every input gradient and every grouped direction gradient inside its own budget, taken from what the DEVICE produced in front of it; bit for bit
on provably exact cases; sentinels, determinism, row independence, the empty call; the ray stages against float64 statements and float64 autograd; the
sanity gate against torch's f32 autograd; the Python layer (parameter gradients unchanged, frozen parameters, render_rays composed by hand, graph
capture) and a pose recovered through the frozen blocks.

Measured on the MI355X when this file was written: see LABBOOK R23."""
import functools

import numpy as np
import pytest
import torch

from nerficg_amd import _lib, nerf
from tests import nerf_grad_ref as B
from tests import nerf_input_grad_ref as I
from tests import nerf_mlp_ref as R
from tests import nerf_rays_ref as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = {'yaml': (8, (5,)), 'one_layer': (1, ()), 'two_skips': (4, (1, 2))}
ENCODINGS = {'k10_4_append': (10, 4, True), 'k10_4_plain': (10, 4, False), 'identity': (0, 0, True)}
SIZES = [1, 127, 128, 129, 273]
PAD = 256


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _guarded(shape, value=-7.0):
    """a device buffer of `shape` with PAD sentinel floats on either side -> (whole, view)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), value, dtype=torch.float32, device=DEV)
    return whole, whole[PAD:PAD + n].view(*shape)


def _untouched(whole, value=-7.0):
    return bool((whole[:PAD] == value).all()) and bool((whole[-PAD:] == value).all())


def device_run(block, pos, rays, dir_group, d_sigma, d_rgb, grad_scale=0.0, sigma_in=None, rgb_in=None):
    """The C ABI directly: training forward, backward, every gradient stage, then the input gradient with its test outputs -- as numpy float64; the
    sentinels around its four outputs are checked, and that it left the gradient stages as it found them."""
    lib, cfg, m = _lib.load(), nerf.fused_config(block), pos.shape[0]
    net = R.net_from_block(block)
    with torch.no_grad():
        blob, blob_t = nerf._train_blobs(block, cfg, torch.device(DEV))
        blob_i = nerf._input_blob(block, cfg, torch.device(DEV))
    assert blob_i.numel() == lib.nrc_nerf_packed_input_bytes(*cfg)
    ws = torch.empty(lib.nrc_nerf_train_workspace_bytes(*cfg, m), dtype=torch.uint8, device=DEV)
    grad = torch.empty(lib.nrc_nerf_grad_params_floats(*cfg), device=DEV)
    stats = torch.empty(4, dtype=torch.int32, device=DEV)
    p, d = _dev(pos), _dev(rays)
    assert d.shape[0] == -(-m // dir_group)
    sigma, rgb = torch.empty(m, device=DEV), torch.empty(m, 3, device=DEV)
    stream = _lib.stream_of(p)
    _lib.check(lib.nrc_nerf_block_forward_train(_lib.ptr(p), _lib.ptr(d), dir_group, m, _lib.ptr(blob), *cfg, _lib.ptr(sigma), _lib.ptr(rgb), _lib.ptr(ws), stream), 'forward_train')
    s_in = sigma if sigma_in is None else _dev(sigma_in)
    r_in = rgb if rgb_in is None else _dev(rgb_in)
    ds, dr = _dev(d_sigma), _dev(d_rgb)
    _lib.check(lib.nrc_nerf_block_backward(_lib.ptr(ds), _lib.ptr(dr), _lib.ptr(s_in), _lib.ptr(r_in), m, _lib.ptr(blob_t), *cfg, _lib.ptr(ws), float(grad_scale),
                                           _lib.ptr(grad), _lib.ptr(stats), stream), 'backward')

    def stages():
        out = {}
        for g, name in enumerate(B.BACKWARD_ORDER(net)):
            width = {'rgb': 3, 'sigma': 1, 'C_1': cfg[0] // 2}.get(name, cfg[0])
            buf = torch.empty(m, width, dtype=torch.float16, device=DEV)
            _lib.check(lib.nrc_nerf_grad_stage(_lib.ptr(ws), *cfg, m, g, _lib.ptr(buf), stream), 'grad_stage')
            out[name] = buf.cpu().numpy().astype(np.float64)
        return out
    G = stages()
    n_pos, n_dir = nerf.fused_tap_names(cfg)[0][1], nerf.fused_tap_names(cfg)[1][1]
    bufs = {'d_positions': _guarded((m, 3)), 'd_directions': _guarded((d.shape[0], 3)), 'dE_pos': _guarded((m, n_pos)), 'dE_dir': _guarded((m, n_dir))}
    _lib.check(lib.nrc_nerf_block_input_grad(_lib.ptr(p), _lib.ptr(d), dir_group, m, _lib.ptr(blob_i), *cfg, _lib.ptr(ws), float(grad_scale),
                                             _lib.ptr(bufs['d_positions'][1]), _lib.ptr(bufs['d_directions'][1]), _lib.ptr(bufs['dE_pos'][1]),
                                             _lib.ptr(bufs['dE_dir'][1]), stream), 'input_grad')
    out = {k: v[1].cpu().numpy().astype(np.float64) for k, v in bufs.items()}
    assert all(_untouched(v[0]) for v in bufs.values()), 'sentinels around the input gradient\'s outputs'
    assert all(np.isfinite(v).all() for v in out.values())
    after = stages()
    assert all(np.array_equal(G[k], after[k]) for k in G), 'the input gradient changed a gradient stage'
    out.update(G=G, e=int(stats[0]), net=net, sigma=sigma.cpu().numpy(), rgb=rgb.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def _random_block(width, shape, enc='k10_4_append', seed=4):
    """default initialisation, the density bias centred on the inputs of R.random_inputs(273, seed=6)"""
    n_layers, skips = SHAPES[shape]
    torch.manual_seed(seed)
    block = nerf.NeRFBlock(n_layers, 1, width, *ENCODINGS[enc], skips)
    net = B.centre_density(R.net_from_block(block), *R.random_inputs(273, seed=6))
    return R.block_from_net(net, DEV)


def _over(res):
    return {k: v for k, v in res.items() if v[0]}


# ------------------------------------------------------------------------------------------------ the block kernel
@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('enc', list(ENCODINGS))
@pytest.mark.parametrize('m', SIZES)
def test_every_element_lies_within_its_budget(width, shape, enc, m):
    """dir_group in {1, 25, M}: a group of 25 straddles the 128-row tiles and ends partial.  The grouped run's per-row values are those of a dir_group = 1
    run on the expanded directions: the device's stated summation of them gives the grouped result bit for bit."""
    block = _random_block(width, shape, enc)
    pos, dirs = R.random_inputs(m, seed=6)
    d_sigma, d_rgb = B.random_upstream(m, seed=6)
    one = device_run(block, pos, dirs, 1, d_sigma, d_rgb)
    res = I.chained_check(one['net'], one['G'], pos, dirs, one['e'], 1, {**one, 'dir_rows': one['d_directions']})
    print(f'W={width} {shape} {enc} M={m} e={one["e"]} dir_group=1: ' + ' '.join(f'{k}={v[1]:.3f}' for k, v in res.items()))
    assert not _over(res)
    assert m < 127 or (np.count_nonzero(one['d_positions']) and np.count_nonzero(one['d_directions']))
    for g in sorted({25, m} - {1}):
        rays = dirs[:-(-m // g)]
        rows = device_run(block, pos, I.row_directions(rays, m, g), 1, d_sigma, d_rgb)
        grouped = device_run(block, pos, rays, g, d_sigma, d_rgb)
        assert grouped['e'] == rows['e'] and all(np.array_equal(grouped[k], rows[k]) for k in ('dE_pos', 'dE_dir', 'd_positions'))
        assert np.array_equal(grouped['d_directions'], I.group_sums_f32(rows['d_directions'], g))
        res = I.chained_check(grouped['net'], grouped['G'], pos, rays, grouped['e'], g, {**grouped, 'dir_rows': rows['d_directions']})
        assert not _over(res), g


def _exact_cases():
    return [(w, s, k, m) for w in (128, 256) for s, k in (('yaml', 0), ('one_layer', 0), ('two_skips', 0), ('yaml', 10), ('zero_family', 10)) for m in (129, 273)]


@pytest.mark.parametrize('width,shape,k_pos,m', _exact_cases())
def test_exact_cases_bit_for_bit(width, shape, k_pos, m):
    net = R.exact_net(width, 'zero') if shape == 'zero_family' else B.exact_net(width, *SHAPES[shape], k_pos, 4 if k_pos else 0)
    block = R.block_from_net(net, DEV)
    pos, dirs = R.exact_inputs(m, 'identity' if k_pos == 0 else 'zero')
    d_sigma, d_rgb, sigma, rgb = B.exact_upstream(m)
    fw = R.forward(net, pos, dirs)
    bw = B.backward(net, fw, sigma, rgb, d_sigma, d_rgb, 4.0)
    for g in ((1,) if k_pos == 0 else (1, 25, m)):       # the identity family's directions differ from row to row
        rays = dirs[:-(-m // g)]
        assert I.exact(net, bw['G'], pos, rays, 4.0, g)
        ref = I.input_gradients(net, bw['G'], pos, rays, 4.0, g)
        got = device_run(block, pos, rays, g, d_sigma, d_rgb, grad_scale=4.0, sigma_in=sigma, rgb_in=rgb)
        assert B.exact_check(bw, {'G': got['G'], 'dW': bw['dW'], 'db': bw['db']}) == []
        if g == 1:
            got['dir_rows'] = got['d_directions']
        assert I.exact_check(ref, got) == [], g
        assert np.count_nonzero(ref['d_positions']) and np.count_nonzero(ref['d_directions'])


@pytest.mark.parametrize('width', [128, 256])
def test_sentinels_two_calls_and_row_independence(width):
    """M = 129 (one row in the second workgroup): the bytes around d_positions / d_directions stay (device_run checks them on every call); two calls
    give the same bits; a row's gradient does not depend on the batch or the grouping."""
    block = _random_block(width, 'yaml')
    pos, dirs = R.random_inputs(273, seed=6)
    d_sigma, d_rgb = B.random_upstream(273, seed=6)
    S = 2.0 ** 14
    a, b = (device_run(block, pos[:129], dirs[:129], 1, d_sigma[:129], d_rgb[:129]) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in ('d_positions', 'd_directions', 'dE_pos', 'dE_dir'))
    rays = dirs[:6]
    a, b = (device_run(block, pos[:129], rays, 25, d_sigma[:129], d_rgb[:129]) for _ in range(2))
    assert np.array_equal(a['d_positions'], b['d_positions']) and np.array_equal(a['d_directions'], b['d_directions'])
    whole = device_run(block, pos, dirs, 1, d_sigma, d_rgb, grad_scale=S)
    for row in (0, 131, 272):
        alone = device_run(block, pos[row:row + 1], dirs[row:row + 1], 1, d_sigma[row:row + 1], d_rgb[row:row + 1], grad_scale=S)
        assert all(np.array_equal(alone[k][0], whole[k][row]) for k in ('d_positions', 'd_directions', 'dE_pos', 'dE_dir')), row
    rays = dirs[:5]                                                # 5 rays x 64 samples, the last one cut short
    grouped = device_run(block, pos, rays, 64, d_sigma, d_rgb, grad_scale=S)
    expanded = device_run(block, pos, I.row_directions(rays, 273, 64), 1, d_sigma, d_rgb, grad_scale=S)
    assert np.array_equal(grouped['d_positions'], expanded['d_positions']) and np.array_equal(grouped['dE_dir'], expanded['dE_dir'])


def test_an_empty_call_launches_nothing():
    block = _random_block(128, 'yaml')
    lib, cfg = _lib.load(), nerf.fused_config(block)
    x = torch.zeros(1024, device=DEV)
    with _lib.stage_timer() as timer:
        assert lib.nrc_nerf_block_input_grad(None, None, 1, 0, None, *cfg, None, 0.0, None, None, None, None, _lib.stream_of(x)) == 0
        assert lib.nrc_nerf_positions_backward(None, None, 0, 64, None, None, _lib.stream_of(x)) == 0
        assert lib.nrc_nerf_integrate_backward_dirs(*([None] * 8), 1e10, 0, 64, None, None, None, _lib.stream_of(x)) == 0
    assert len(timer.stages) == 0
    assert lib.nrc_nerf_block_input_grad(_lib.ptr(x), _lib.ptr(x), 0, 5, _lib.ptr(x), *cfg, _lib.ptr(x), 0.0, _lib.ptr(x), _lib.ptr(x), None, None, None) == -1


@pytest.mark.parametrize('width', [128, 256])
def test_sanity_gate_against_torch_f32_autograd(width):
    """C = max |restatement - torch f32 autograd| for pos.grad and for dirs.grad (what fp16 operands and gradients cost by themselves); the device stays
    within 2 C."""
    block = _random_block(width, 'yaml')
    m = 273
    pos, dirs = R.random_inputs(m, seed=12)
    d_sigma, d_rgb = B.random_upstream(m, seed=12)
    got = device_run(block, pos, dirs, 1, d_sigma, d_rgb)
    net = got['net']
    fw = R.forward(net, pos, dirs)
    S = 2.0 ** got['e']
    ref = I.input_gradients(net, B.backward(net, fw, fw['sigma'], fw['rgb'], d_sigma, d_rgb, S)['G'], pos, dirs, S)
    p, d = _dev(pos).requires_grad_(), _dev(dirs).requires_grad_()
    sigma, rgb = block(p, d)
    ((sigma[:, 0] * _dev(d_sigma)).sum() + (rgb * _dev(d_rgb)).sum()).backward()
    for name, t, r, g in (('pos', p.grad, ref['d_positions'], got['d_positions']), ('dirs', d.grad, ref['d_directions'], got['d_directions'])):
        t = t.double().cpu().numpy()
        c, e = np.abs(r - t).max(), np.abs(g - t).max()
        print(f'W={width} {name}.grad: C = {c:.3e}, device vs torch {e:.3e} ({e / c:.3f} C), largest |grad| {np.abs(t).max():.3e}')
        assert c > 0 and e <= 2.0 * c, (name, e, c)


# ------------------------------------------------------------------------------------------------ the ray stages
def _ray_case(n, s, seed=0):
    rng = np.random.default_rng([seed, n, s])
    t = np.sort(rng.uniform(2.0, 6.0, size=(n, s)), axis=-1).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    sigma = (rng.uniform(0.0, 3.0, size=(n, s)) * (rng.uniform(size=(n, s)) < 0.7)).astype(np.float32)
    sigma[0, -1] = 0.0                                              # ray 0: the last segment stays open (sigma_last = 0)
    if n > 1:
        sigma[1, -1] = 0.75                                         # ray 1: sigma_last > 0 against final_delta = 1e10
        d[2] = 0.0                                                  # ray 2: |d| = 0
    c = rng.uniform(size=(n, s, 3)).astype(np.float32)
    bg = np.array([1.0, 0.5, 0.25], np.float32)
    up = (rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=n).astype(np.float32), (rng.normal(size=(n, s)) * 0.1).astype(np.float32))
    return t, d, sigma, c, bg, up


@pytest.mark.parametrize('s', [1, 3, 64, 65, 256, 1024])
@pytest.mark.parametrize('n', [1, 5])
def test_ray_stages_within_their_budgets(n, s):
    """Five rays: one full four-ray workgroup plus one.  The |d| term against float64 torch autograd through nerf.integrate_samples."""
    lib = _lib.load()
    t, d, sigma, c, bg, up = _ray_case(n, s)
    if n == 1:
        sigma[0, -1] = 0.75 if s % 2 else 0.0
    g = np.random.default_rng([3, n, s]).normal(size=(n * s, 3)).astype(np.float32)
    tt, gg = _dev(t), _dev(g)
    (w_o, d_o), (w_d, d_d) = _guarded((n, 3)), _guarded((n, 3))
    stream = _lib.stream_of(tt)
    _lib.check(lib.nrc_nerf_positions_backward(_lib.ptr(gg), _lib.ptr(tt), n, s, _lib.ptr(d_o), _lib.ptr(d_d), stream), 'positions_backward')
    assert _untouched(w_o) and _untouched(w_d)
    (ref_o, b_o), (ref_d, b_d) = I.positions_backward_budget(g, t)
    assert np.all(np.abs(d_o.double().cpu().numpy() - ref_o) <= b_o) and np.all(np.abs(d_d.double().cpu().numpy() - ref_d) <= b_d)
    assert np.abs(ref_d).max() > 0
    # the compositor's backward with the direction term
    dd, ss, cc, bb = _dev(d), _dev(sigma), _dev(c), _dev(bg)
    ups = [_dev(a) for a in up]
    plain = (torch.empty(n, s, device=DEV), torch.empty(n, s, 3, device=DEV))
    _lib.check(lib.nrc_nerf_integrate_backward(*[_lib.ptr(a) for a in ups], _lib.ptr(tt), _lib.ptr(dd), _lib.ptr(ss), _lib.ptr(cc), _lib.ptr(bb), 1e10, n, s,
                                               _lib.ptr(plain[0]), _lib.ptr(plain[1]), stream), 'integrate_backward')
    (w_s, d_s), (w_c, d_c), (w_dir, d_dir) = _guarded((n, s)), _guarded((n, s, 3)), _guarded((n, 3))
    _lib.check(lib.nrc_nerf_integrate_backward_dirs(*[_lib.ptr(a) for a in ups], _lib.ptr(tt), _lib.ptr(dd), _lib.ptr(ss), _lib.ptr(cc), _lib.ptr(bb), 1e10, n, s,
                                                    _lib.ptr(d_s), _lib.ptr(d_c), _lib.ptr(d_dir), stream), 'integrate_backward_dirs')
    assert _untouched(w_s) and _untouched(w_c) and _untouched(w_dir)
    assert torch.equal(d_s, plain[0]) and torch.equal(d_c, plain[1])
    got = d_dir.double().cpu().numpy()
    assert np.isfinite(got).all()
    fw = Y.integrate_f64(t, d, sigma, c, bg, 1e10)
    aux = Y.integrate_backward_f64(fw, *up)[2]
    stated, bound = I.dirs_budget(fw, aux, d, sigma, 1e10, Y.backward_budget(fw, aux)[0])
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))    # noqa: E731
    d64 = t64(d).requires_grad_()
    rgb, _, alpha, w = nerf.integrate_samples(t64(t), d64, t64(sigma), t64(c), t64(bg), 1e10)
    ((rgb * t64(up[0])).sum() + (alpha[:, 0] * t64(up[1])).sum() + (w * t64(up[2])).sum()).backward()
    ref = d64.grad.numpy()
    assert np.abs(stated - ref).max() <= 1e-11 * max(np.abs(ref).max(), 1e-300)
    ratio, over = I.judge(got, ref, bound)
    print(f'N={n} S={s}: |d| term worst error / bound {ratio:.3f}, largest |value| {np.abs(ref).max():.3e}')
    assert over == 0
    if n > 1:
        assert not got[2].any() and (s == 1 or np.abs(ref[[0, 1, 3, 4]]).max() > 0)       # (a short ray's random densities may all be 0)


# ------------------------------------------------------------------------------------------------ the Python layer
def _fresh_block(seed=2, n_layers=4, width=128, **kw):
    torch.manual_seed(seed)
    block = nerf.NeRFBlock(n_layers, 1, width, **kw).to(DEV)
    with torch.no_grad():
        block.density_layer.bias.fill_(0.5)
    return block


def test_fused_apply_returns_the_c_calls_gradients_and_keeps_the_parameters_bits():
    block = _fresh_block()
    m, g = 200, 25
    pos_np, dirs_np = R.random_inputs(m, seed=3)
    rays_np = dirs_np[:m // g]
    w1 = np.linspace(0.5, 1.5, m).astype(np.float32) * 1e-3
    w3 = np.linspace(-1.0, 1.0, 3 * m).astype(np.float32).reshape(m, 3) * 1e-3

    def run(flag, frozen=False):
        for q in block.parameters():
            q.requires_grad_(not frozen)
        block.zero_grad(set_to_none=True)
        pos, rays = _dev(pos_np).requires_grad_(flag), _dev(rays_np).requires_grad_(flag)
        with _lib.stage_timer() as timer:
            sigma, rgb = nerf.fused_apply(block, pos, rays, dir_group=g, input_grad=flag)
            ((sigma[:, 0] * _dev(w1)).sum() + (rgb * _dev(w3)).sum()).backward()
        return [None if q.grad is None else q.grad.clone() for q in block.parameters()], pos.grad, rays.grad, [n for n, _ in timer.stages]
    plain, none_p, none_r, _ = run(False)
    assert none_p is None and none_r is None
    with_flag, gp, gr, names = run(True)
    assert all(torch.equal(a, b) for a, b in zip(plain, with_flag))
    assert names[-2:] == ['k_nerf_input_grad', 'k_nerf_dir_reduce'] and 'k_nerf_pack_i' in names
    want = device_run(block, pos_np, rays_np, g, w1, w3)
    assert np.array_equal(gp.double().cpu().numpy(), want['d_positions']) and np.array_equal(gr.double().cpu().numpy(), want['d_directions'])
    assert np.count_nonzero(want['d_positions']) and np.count_nonzero(want['d_directions'])
    frozen, fp, fr, names = run(True, frozen=True)          # tracking against a frozen model: the device path still runs
    assert all(q is None for q in frozen) and torch.equal(fp, gp) and torch.equal(fr, gr)
    assert 'k_nerf_forward_train' in names and 'k_nerf_input_grad' in names and block._fused_cache['packs_i'] == 1
    for q in block.parameters():
        q.requires_grad_(True)


def _rays(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=gen) * 0.3
    d = torch.randn(n, 3, generator=gen)
    return o.to(DEV), d.to(DEV), (d / d.norm(dim=-1, keepdim=True)).to(DEV)


@pytest.mark.parametrize('with_coarse', [True, False])
def test_render_rays_composes_the_c_calls_outputs(with_coarse, monkeypatch):
    """origin.grad = sum over the passes of sum_s g_s; direction.grad = sum over the passes of sum_s t_s g_s + the compositor's direction term;
    view_direction.grad = sum over the passes of the block's grouped direction gradient -- against float64 sums of the hooked per-pass gradients, within
    the summation budgets of tests/nerf_input_grad_ref.py plus autograd's own additions of the passes."""
    coarse, fine = _fresh_block(5), _fresh_block(6, 8, 256)
    o, d, vd = (a.requires_grad_() for a in _rays(40, seed=1))
    seen = []
    apply_, composite_ = nerf.fused_apply, nerf.composite

    def spy_apply(block, pos, dirs, **kw):
        dirs = dirs.view_as(dirs)                                      # a node of its own: the hook sees this pass alone
        entry = {}
        seen.append(entry)
        pos.register_hook(lambda g: entry.__setitem__('g_pos', g.detach().double().cpu().numpy()))
        dirs.register_hook(lambda g: entry.__setitem__('g_view', g.detach().double().cpu().numpy()))
        assert kw.get('input_grad') is True
        return apply_(block, pos, dirs, **kw)

    def spy_composite(t, dirs, *rest, **kw):
        dirs = dirs.view_as(dirs)
        seen[-1]['t'] = t.detach().double().cpu().numpy()
        dirs.register_hook(lambda g, entry=seen[-1]: entry.__setitem__('g_len', g.detach().double().cpu().numpy()))
        assert kw.get('input_grad') is True
        return composite_(t, dirs, *rest, **kw)
    monkeypatch.setattr(nerf, 'fused_apply', spy_apply)
    monkeypatch.setattr(nerf, 'composite', spy_composite)
    with _lib.stage_timer() as timer:
        out = nerf.render_rays(coarse if with_coarse else None, fine, o, d, vd, 2.0, 6.0, torch.tensor([1.0, 0.5, 0.25]), n_samples_coarse_nerf=16,
                               n_samples_nerf=48, fused_train=True, device_rays=True, input_grad=True)
        w = torch.rand(40, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
        ((out['rgb'] * w).sum() + ((out['rgb_coarse'] * w).sum() if with_coarse else 0.0) + out['alpha'].sum()).backward()
    names = [n for n, _ in timer.stages]
    n_pass = 2 if with_coarse else 1
    assert len(seen) == n_pass and all(k in e for e in seen for k in ('g_pos', 'g_view', 'g_len', 't'))
    assert names.count('k_nerf_input_grad') == n_pass and names.count('k_nerf_positions_bw') == n_pass and names.count('k_nerf_integrate_bw_dirs') == n_pass
    assert 'k_nerf_integrate_bw' not in names and names.count('k_nerf_dgrad') == n_pass           # nothing fell back
    want_o, want_d, want_v, tol_o, tol_d, tol_v = (np.zeros((40, 3)) for _ in range(6))
    for e in seen:
        (d_o, b_o), (d_d, b_d) = I.positions_backward_budget(e['g_pos'], e['t'])
        want_o, want_d, want_v = want_o + d_o, want_d + d_d + e['g_len'], want_v + e['g_view']
        # autograd adds at most four terms into a leaf's .grad: three additions, each within u of a partial sum that the sum of |terms| bounds; 4 u of slack
        tol_o, tol_d = tol_o + b_o + 4.0 * I.U * np.abs(d_o), tol_d + b_d + 4.0 * I.U * (np.abs(d_d) + np.abs(e['g_len']))
        tol_v = tol_v + 4.0 * I.U * np.abs(e['g_view'])
    for name, got, want, tol in (('origin', o.grad, want_o, tol_o), ('direction', d.grad, want_d, tol_d), ('view_direction', vd.grad, want_v, tol_v)):
        assert np.abs(want).max() > 0 and np.all(np.abs(got.double().cpu().numpy() - want) <= tol), name
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in fine.parameters())


def test_forward_and_backward_capture_into_one_graph():
    block = _fresh_block(8)
    m, g = 300, 25
    pos_np, dirs_np = R.random_inputs(m, seed=4)
    pos, rays = _dev(pos_np).requires_grad_(), _dev(dirs_np[:m // g]).requires_grad_()
    w = torch.rand(m, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    out_p, out_r = torch.zeros(m, 3, device=DEV), torch.zeros(m // g, 3, device=DEV)

    def step():
        sigma, rgb = nerf.fused_apply(block, pos, rays, dir_group=g, input_grad=True)
        gp, gr = torch.autograd.grad((rgb * w).sum() + sigma.mean() * 1e-3, (pos, rays))
        out_p.copy_(gp)
        out_r.copy_(gr)
    step()
    eager = out_p.clone(), out_r.clone()
    assert float(eager[0].abs().sum()) > 0 and float(eager[1].abs().sum()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    del block.__dict__['_fused_cache']                # the capture records the three packs
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    out_p.zero_()
    out_r.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_p, eager[0]) and torch.equal(out_r, eager[1])


# ------------------------------------------------------------------------------------------------ behaviour
def _pose_scene():
    """Two frozen 4 x 128 blocks with K_pos = 2 (a smooth field), weights three times the default initialisation (so that the picture changes by about
    0.1 over the offset below) and an open density head; a 16 x 16 pinhole fan of rays from one camera position."""
    torch.manual_seed(11)
    blocks = [nerf.NeRFBlock(4, 1, 128, 2, 1, True, (2,)).to(DEV) for _ in range(2)]
    with torch.no_grad():
        for b in blocks:
            for lin in nerf._block_linears(b):
                lin.weight.mul_(3.0)
            b.density_layer.bias.fill_(0.5)
            for q in b.parameters():
                q.requires_grad_(False)
    ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, 16), torch.linspace(-0.5, 0.5, 16), indexing='ij')
    d = torch.stack([xs.flatten(), ys.flatten(), -torch.ones(256)], dim=1).to(DEV).contiguous()
    return blocks[0], blocks[1], d, (d / d.norm(dim=-1, keepdim=True)).contiguous()


def _recover(coarse, fine, d, vd, target, start, steps, **kw):
    c = start.clone().requires_grad_()
    opt = torch.optim.Adam([c], lr=0.01)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        out = nerf.render_rays(coarse, fine, c[None, :].expand(256, 3).contiguous(), d, vd, 0.5, 3.0, torch.ones(3), n_samples_coarse_nerf=16,
                               n_samples_nerf=32, **kw)
        ((out['rgb'] - target['rgb']).square().mean() + (out['rgb_coarse'] - target['rgb_coarse']).square().mean()).backward()
        opt.step()
    return c.detach()


def test_a_camera_translation_is_recovered_through_the_frozen_blocks():
    """The target is rendered by the torch path from a known position; the camera starts 0.112 away; 120 Adam steps.  The torch f32 path, run here as the
    reference, must end within 0.05 of the initial offset (the scene was chosen so), the fused path with input_grad=True within 0.1 of it.
    Measured on the MI355X (LABBOOK R23): torch f32 0.0004, fused 0.0015 of the initial offset."""
    coarse, fine, d, vd = _pose_scene()
    c0 = torch.tensor([0.1, -0.05, 1.5], device=DEV)
    offset = torch.tensor([0.06, -0.08, 0.05], device=DEV)
    with torch.no_grad():
        target = nerf.render_rays(coarse, fine, c0[None, :].expand(256, 3).contiguous(), d, vd, 0.5, 3.0, torch.ones(3), n_samples_coarse_nerf=16, n_samples_nerf=32)
    e_torch = float((_recover(coarse, fine, d, vd, target, c0 + offset, 120) - c0).norm() / offset.norm())
    with _lib.stage_timer() as timer:
        e_fused = float((_recover(coarse, fine, d, vd, target, c0 + offset, 120, fused_train=True, device_rays=True, input_grad=True) - c0).norm() / offset.norm())
    names = [n for n, _ in timer.stages]
    print(f'camera error / initial offset after 120 steps: torch f32 {e_torch:.4f}, fused with input_grad {e_fused:.4f}')
    assert names.count('k_nerf_input_grad') == 240 and names.count('k_nerf_positions_bw') == 240          # the fused path ran, both passes, every step
    assert e_torch <= 0.05
    assert e_fused <= 0.1
