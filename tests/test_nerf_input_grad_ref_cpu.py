"""CPU: tests/nerf_input_grad_ref.py checks itself -- with every rounding switched off its d_positions / d_directions are float64 torch autograd through
an f64 NeRFBlock (so the restatement is the true derivative), its exact cases are exact, each planted defect breaks at least one element's budget, an f32
emulation with the forward's own sin / cos stays inside the budget, and the two ray-stage statements are held against float64 autograd and their own
planted defects.  Plus what of C ABI group 20 can be checked without a GPU: the version, the exports and the argument validation.  None of this pins the
device: tests/test_gpu_nerf_input_grad.py does."""
import numpy as np
import pytest
import torch

from nerficg_amd import _lib, nerf
from tests import nerf_grad_ref as B
from tests import nerf_input_grad_ref as I
from tests import nerf_mlp_ref as R
from tests import nerf_rays_ref as Y

SHAPES = {'yaml': (8, (5,)), 'one_layer': (1, ()), 'two_skips': (4, (1, 2))}
EXPORTS = ('nrc_nerf_packed_input_bytes', 'nrc_nerf_pack_weights_input', 'nrc_nerf_block_input_grad', 'nrc_nerf_positions_backward',
           'nrc_nerf_integrate_backward_dirs')


def _fp16_net(n_layers, skips, width=128, seed=3, m=65):
    """a freshly initialised block whose weights are fp16 numbers already (so that switching the rounding off changes no weight), density centred"""
    torch.manual_seed(seed)
    net = R.net_from_block(nerf.NeRFBlock(n_layers, 1, width, 10, 4, True, skips))
    net = R.make_net([(R.sat(R.h16(w)), b) for w, b in net['lin']], net['L'], 1, net['k_pos'], net['k_dir'], net['append'], net['skips'])
    pos, dirs = R.random_inputs(m, seed=seed)
    return B.centre_density(net, pos, dirs), pos, dirs


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('dir_group', [1, 25])
def test_without_rounding_the_restatement_is_float64_autograd(shape, dir_group):
    m = 65
    net, pos, dirs = _fp16_net(*SHAPES[shape], m=m)
    rays = dirs[:-(-m // dir_group)]
    expanded = I.row_directions(rays, m, dir_group)
    d_sigma, d_rgb = B.random_upstream(m, seed=3)
    block = R.block_from_net(net).double()
    p = torch.from_numpy(pos).double().requires_grad_()
    d = torch.from_numpy(rays).double().requires_grad_()
    sigma, rgb = block(p, d[torch.arange(m) // dir_group])
    ((sigma[:, 0] * torch.from_numpy(d_sigma).double()).sum() + (rgb * torch.from_numpy(d_rgb).double()).sum()).backward()
    fw = R.forward(net, pos, expanded, rounding=False)
    assert np.abs(fw['sigma'] - sigma[:, 0].detach().numpy()).max() <= 1e-12 and (fw['sigma'] > 0).any()
    bw = B.backward(net, fw, fw['sigma'], fw['rgb'], d_sigma, d_rgb, 1.0, rounding=False)
    out = I.input_gradients(net, bw['G'], pos, rays, 1.0, dir_group, rounding=False)
    for got, ref in ((out['d_positions'], p.grad.numpy()), (out['d_directions'], d.grad.numpy())):
        assert ref.shape == got.shape and np.abs(ref).max() > 0
        assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max()


def _random_case(n_layers=8, skips=(2, 5), m=273, seed=3, e=14, dir_group=25):
    torch.manual_seed(seed)
    net = R.net_from_block(nerf.NeRFBlock(n_layers, 1, 128, 10, 4, True, skips))
    pos, dirs = R.random_inputs(m, seed=seed)
    rays = dirs[:-(-m // dir_group)]
    expanded = I.row_directions(rays, m, dir_group)
    net = B.centre_density(net, pos, expanded)
    fw = R.forward(net, pos, expanded)
    d_sigma, d_rgb = B.random_upstream(m, seed=seed)
    G = B.backward(net, fw, fw['sigma'].astype(np.float32), fw['rgb'].astype(np.float32), d_sigma, d_rgb, 2.0 ** e)['G']
    return net, G, pos, rays, e, dir_group


def _over(res):
    return {k: v for k, v in res.items() if v[0]}


@pytest.mark.parametrize('mut', I.MUTATIONS)
def test_each_planted_defect_breaks_a_budget(mut):
    net, G, pos, rays, e, g = _random_case()
    good = I.input_gradients(net, G, pos, rays, 2.0 ** e, g)
    assert np.count_nonzero(good['d_positions']) and np.count_nonzero(good['d_directions'])
    assert not _over(I.chained_check(net, G, pos, rays, e, g, good))
    bad = I.input_gradients(net, G, pos, rays, 2.0 ** e, g, mut=mut)
    assert _over(I.chained_check(net, G, pos, rays, e, g, bad)), f'{mut}: inside every budget'


def test_an_f32_device_with_the_forwards_sincos_stays_inside_the_dx_budget():
    net, G, pos, rays, e, g = _random_case()
    dE = I.enc_gradients(net, G)['pos']['Z'].astype(np.float32).astype(np.float64)
    ref, bound = I.dx_budget(pos, dE, net['k_pos'], net['append'], e)
    got = I.dx_f32_model(pos, dE, net['k_pos'], net['append'], e)
    ratio, over = I.judge(got, ref, bound)
    assert over == 0 and 0.0 < ratio < 1.0
    assert np.abs(pos).max() <= 8.0 and net['k_pos'] - 1 <= 9          # the domain E_ENC is stated for


@pytest.mark.parametrize('width', [128, 256])
@pytest.mark.parametrize('shape,k_pos', [('yaml', 0), ('one_layer', 0), ('two_skips', 0), ('yaml', 10), ('zero_family', 10)])
def test_exact_cases_are_exact(width, shape, k_pos):
    m, g = 273, 25
    net = R.exact_net(width, 'zero') if shape == 'zero_family' else B.exact_net(width, *SHAPES[shape], k_pos, 4 if k_pos else 0)
    pos, dirs = R.exact_inputs(m, 'identity' if k_pos == 0 else 'zero')
    fw = R.forward(net, pos, dirs)
    d_sigma, d_rgb, sigma, rgb = B.exact_upstream(m)
    bw = B.backward(net, fw, sigma, rgb, d_sigma, d_rgb, 4.0)
    assert R.exact(net, pos, dirs, fw)[0] and B.exact(net, fw, sigma, rgb, d_sigma, d_rgb, 4.0, bw=bw)[0]
    for group, rays in ((1, dirs), (g, dirs[:-(-m // g)] if k_pos else None)):
        if rays is None:        # the identity family's directions differ from row to row: grouped, the forward would see other rows
            continue
        assert I.exact(net, bw['G'], pos, rays, 4.0, group)
        out = I.input_gradients(net, bw['G'], pos, rays, 4.0, group)
        assert np.count_nonzero(out['d_positions']) and np.count_nonzero(out['d_directions'])      # not exact because it is empty


# ------------------------------------------------------------------------------------------------ the ray stages
def _ray_case(n=5, s=65, seed=0, final_delta=1e10):
    rng = np.random.default_rng([seed, n, s])
    t = np.sort(rng.uniform(2.0, 6.0, size=(n, s)), axis=-1).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    sigma = (rng.uniform(0.0, 3.0, size=(n, s)) * (rng.uniform(size=(n, s)) < 0.7)).astype(np.float32)
    sigma[0, -1], sigma[1 % n, -1] = 0.0, 0.75                      # the last segment closed and open
    if n > 2:
        d[2] = 0.0                                                  # a ray without a direction
    c = rng.uniform(size=(n, s, 3)).astype(np.float32)
    bg = np.array([1.0, 0.5, 0.25], np.float32)
    up = (rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=n).astype(np.float32), (rng.normal(size=(n, s)) * 0.1).astype(np.float32))
    return t, d, sigma, c, bg, up, final_delta


def _autograd_dirs(t, d, sigma, c, bg, up, final_delta):
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    dd = t64(d).requires_grad_()
    rgb, _, alpha, w = nerf.integrate_samples(t64(t), dd, t64(sigma), t64(c), t64(bg), final_delta)
    ((rgb * t64(up[0])).sum() + (alpha[:, 0] * t64(up[1])).sum() + (w * t64(up[2])).sum()).backward()
    return dd.grad.numpy()


@pytest.mark.parametrize('s', [1, 3, 65])
@pytest.mark.parametrize('final_delta', [1e10, 0.5])
def test_the_direction_term_of_the_compositor_is_float64_autograd(s, final_delta):
    t, d, sigma, c, bg, up, fd = _ray_case(s=s, final_delta=final_delta)
    fw = Y.integrate_f64(t, d, sigma, c, bg, fd)
    aux = Y.integrate_backward_f64(fw, *up)[2]
    got, _ = I.dirs_term_f64(fw, aux, d, sigma, fd)
    ref = _autograd_dirs(t, d, sigma, c, bg, up, fd)
    assert np.isfinite(got).all() and np.isfinite(ref).all() and not got[2].any() and not ref[2].any()
    assert np.abs(got - ref).max() <= 1e-11 * max(np.abs(ref).max(), 1e-300) and (s == 1 and final_delta > 1 or np.abs(ref).max() > 0)


@pytest.mark.parametrize('mut', I.RAY_MUTATIONS)
def test_each_planted_defect_of_the_ray_stages_breaks_a_budget(mut):
    t, d, sigma, c, bg, up, fd = _ray_case(final_delta=0.5)
    if mut in I.RAY_MUTATIONS[:2]:
        g = np.random.default_rng(4).normal(size=(t.size, 3)).astype(np.float32)
        (d_o, b_o), (d_d, b_d) = I.positions_backward_budget(g, t)
        bad = I.positions_backward_f64(g, t, mut=mut)
        assert np.any(np.abs(bad[0] - d_o) > b_o) or np.any(np.abs(bad[1] - d_d) > b_d)
        f32 = (g.reshape(*t.shape, 3).astype(np.float32) * t[:, :, None]).astype(np.float32)
        assert np.all(np.abs(np.cumsum(f32, axis=1, dtype=np.float32)[:, -1].astype(np.float64) - d_d) <= b_d)        # an f32 order of summation stays inside
        return
    fw = Y.integrate_f64(t, d, sigma, c, bg, fd)
    aux = Y.integrate_backward_f64(fw, *up)[2]
    ref, bound = I.dirs_budget(fw, aux, d, sigma, fd, Y.backward_budget(fw, aux)[0])
    assert np.all(bound[2] == 0.0) and np.all(bound[[0, 1, 3, 4]] > 0.0) and np.all(bound <= 1e-3 * np.abs(ref).max())
    bad, _ = I.dirs_term_f64(fw, aux, d, sigma, fd, mut=mut)
    assert np.any(np.abs(bad - ref) > bound), mut


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_group_20_exports_and_argument_validation():
    lib = _lib.load()
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 19
    protos = _lib.parse_header()
    for name in EXPORTS:
        assert name in protos and hasattr(lib, name), name
    cfg, bad = (256, 8, 1, 10, 4, 1, 32), (256, 8, 2, 10, 4, 1, 32)
    n_pos, n_dir, W = 63, 27, 256
    assert lib.nrc_nerf_packed_input_bytes(*cfg) == 2 * (2 * 32 * W + 2 * 32 * W) + 2 * 32 * (W // 2) > 0      # W_0 and one skip as 2 m-tiles, the colour columns as 1
    assert lib.nrc_nerf_packed_input_bytes(*bad) == -3
    buf = torch.zeros(1024, dtype=torch.float32)       # host memory: every call below must return before it launches anything
    p = _lib.ptr(buf)
    odd4, odd16 = _lib.ctypes.c_void_p(buf.data_ptr() + 2), _lib.ctypes.c_void_p(buf.data_ptr() + 4)
    assert buf.data_ptr() % 16 == 0
    grad = lambda m, g, ptrs, scale=0.0: lib.nrc_nerf_block_input_grad(ptrs[0], ptrs[1], g, m, ptrs[2], *cfg, ptrs[3], scale, *ptrs[4:], None)     # noqa: E731
    nul, ok = [None] * 8, [p] * 8
    assert grad(0, 1, nul) == 0 and grad(-1, 1, nul) == -1 and grad(5, 1, nul) == -1 and grad(5, 0, ok) == -1 and grad(5, -3, ok) == -1
    assert grad(5, 1, ok, scale=3.0) == -1 and grad(5, 1, ok, scale=-2.0) == -1
    assert lib.nrc_nerf_block_input_grad(p, p, 1, 5, p, *bad, p, 0.0, p, p, p, p, None) == -3
    for k in range(8):
        assert grad(5, 1, [(odd16 if k in (2, 3) else odd4) if j == k else p for j in range(8)]) == -1, k
    for k in range(6):                                   # the required pointers, each alone; d_enc_pos / d_enc_dir may be null
        assert grad(5, 1, [None if j == k else p for j in range(8)]) == -1, k
    assert lib.nrc_nerf_pack_weights_input(None, 24, *cfg, p, None) == -1 and lib.nrc_nerf_pack_weights_input(p, 22, *cfg, p, None) == -1
    assert lib.nrc_nerf_pack_weights_input(p, 24, *cfg, odd16, None) == -1 and lib.nrc_nerf_pack_weights_input(p, 24, *bad, p, None) == -3
    pbw = lambda n, s, ptrs: lib.nrc_nerf_positions_backward(ptrs[0], ptrs[1], n, s, ptrs[2], ptrs[3], None)                                       # noqa: E731
    dbw = lambda n, s, ptrs: lib.nrc_nerf_integrate_backward_dirs(*ptrs[:8], 1e10, n, s, *ptrs[8:], None)                                         # noqa: E731
    for call, n_ptrs, required in ((pbw, 4, (0, 1, 2, 3)), (dbw, 11, (3, 4, 5, 6, 8, 9, 10))):
        nul = [None] * n_ptrs
        assert call(0, 64, nul) == 0 and call(-1, 64, nul) == -1 and call(5, 64, nul) == -1
        assert call(0, 0, nul) == -3 and call(0, 1025, nul) == -3 and call(5, 1025, [p] * n_ptrs) == -3
        for k in range(n_ptrs):
            assert call(5, 64, [odd4 if j == k else p for j in range(n_ptrs)]) == -1, (call, k)
        for k in required:
            assert call(5, 64, [None if j == k else p for j in range(n_ptrs)]) == -1, (call, k)


def test_the_default_keeps_every_fallback():
    """input_grad defaults to False on every entry of the Python layer, and on the CPU the flag changes nothing: torch's bits and torch's gradients"""
    import inspect
    for fn in (nerf.fused_apply, nerf.sample_coarse, nerf.sample_fine, nerf.composite, nerf.render_rays):
        assert inspect.signature(fn).parameters['input_grad'].default is False, fn
    torch.manual_seed(1)
    block = nerf.NeRFBlock(2, 1, 128)
    results = []
    for flag in (False, True):
        o, d = (torch.randn(6, 3, generator=torch.Generator().manual_seed(s)).requires_grad_() for s in (1, 2))
        vd = (d / d.norm(dim=-1, keepdim=True)).detach().requires_grad_()
        block.zero_grad(set_to_none=True)
        out = nerf.render_rays(block, block, o, d, vd, 2.0, 6.0, torch.ones(3), n_samples_coarse_nerf=8, n_samples_nerf=8, fused_train=True, device_rays=True,
                               input_grad=flag)
        (out['rgb'].square().sum() + out['rgb_coarse'].square().sum()).backward()
        results.append([out['rgb'].detach(), o.grad, d.grad, vd.grad] + [q.grad for q in block.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*results)) and float(results[0][1].abs().sum()) > 0
