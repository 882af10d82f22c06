"""GPU: the NeRF ray stages (csrc/nerf_rays.hip, header group 19; nerf.sample_coarse / composite / sample_fine / render_rays(device_rays=True)) against
tests/nerf_rays_ref.py -- sampling and resampling bit for bit against the f32 restatement, compositing forward and backward inside per-element budgets
against f64 on the same f32 inputs, the fixtures recorded from the reference's own code, special rays, determinism, ray independence, sentinels, and the
Python layer (autograd, render_rays, fallbacks, graph capture).  Every case is a few dozen rays."""

import numpy as np
import pytest
import torch

from nerficg_amd import _lib, nerf
from tests import nerf_rays_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -77.25
S_LIST = [1, 2, 3, 63, 64, 65, 192, 256, 257, 1024]
FINE_LIST = [(3, 1), (64, 192), (65, 191), (64, 64), (1024, 1024)]


def _rpg():
    return _lib.load().nrc_nerf_rays_per_group()


def _n_list():
    r = _rpg()
    return sorted({1, max(r - 1, 1), r, r + 1, 37, 4 * r + 1})


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


class _Out:
    """an output buffer one element longer than needed, pre-filled with a sentinel that must survive"""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 1,), SENTINEL, dtype=torch.float32, device=DEV)

    def get(self):
        host = self.buf.cpu().numpy()
        assert host[self.n] == np.float32(SENTINEL), 'the element behind the buffer was overwritten'
        return host[:self.n].reshape(self.shape)


def dev_sample_coarse(o, d, t_row, u):
    n, s = o.shape[0], t_row.shape[0]
    t, pos = _Out(n, s), _Out(n * s, 3)
    args = [_dev(o), _dev(d), _dev(t_row), _dev(u)]
    _lib.check(_lib.load().nrc_nerf_sample_coarse(*map(_lib.ptr, args), n, s, _lib.ptr(t.buf), _lib.ptr(pos.buf), _lib.stream_of(args[0])), 'sample_coarse')
    return t.get(), pos.get()


def dev_forward(t, d, sigma, c, bg, fd):
    n, s = t.shape
    outs = [_Out(n, 3), _Out(n), _Out(n), _Out(n, s)]
    args = [_dev(t), _dev(d), _dev(sigma), _dev(c), _dev(bg)]
    _lib.check(_lib.load().nrc_nerf_integrate_forward(*map(_lib.ptr, args), fd, n, s, *[_lib.ptr(x.buf) for x in outs], _lib.stream_of(args[0])), 'forward')
    return dict(zip(('rgb', 'depth', 'alpha', 'weights'), (x.get() for x in outs)))


def dev_backward(up, t, d, sigma, c, bg, fd):
    n, s = t.shape
    outs = [_Out(n, s), _Out(n, s, 3)]
    args = [_dev(x) for x in up] + [_dev(t), _dev(d), _dev(sigma), _dev(c), _dev(bg)]
    _lib.check(_lib.load().nrc_nerf_integrate_backward(*map(_lib.ptr, args), fd, n, s, *[_lib.ptr(x.buf) for x in outs], _lib.stream_of(args[3])), 'backward')
    return outs[0].get(), outs[1].get()


def dev_sample_fine(t_c, w, u, o, d):
    n, sc = t_c.shape
    sf = u.shape[-1]
    outs = [_Out(n, sc + sf), _Out(n * (sc + sf), 3), _Out(n, sc - 1), _Out(n, sf)]
    args = [_dev(t_c), _dev(w), _dev(u)]
    tail = [_dev(o), _dev(d)]
    _lib.check(_lib.load().nrc_nerf_sample_fine(*map(_lib.ptr, args), sf if u.ndim == 2 else 0, *map(_lib.ptr, tail), n, sc, sf,
                                                *[_lib.ptr(x.buf) for x in outs], _lib.stream_of(args[0])), 'sample_fine')
    return dict(zip(('t', 'positions', 'cdf', 't_fine'), (x.get() for x in outs)))


def _rays(n, seed):
    g = np.random.default_rng(seed)
    o = (g.standard_normal((n, 3)) * 0.3).astype(np.float32)
    d = g.standard_normal((n, 3)).astype(np.float32)
    d *= (g.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)      # |d| != 1: the lengths are scaled
    return o, d


def _scene(n, s, seed):
    """random rays with stratified depths; ray 0 empty (sigma = 0), ray 1 saturating (sigma x 40, as in the fixture)"""
    g = np.random.default_rng(seed)
    o, d = _rays(n, seed + 1)
    t_row = torch.linspace(2.0, 6.0, s).numpy()
    t = R.sample_coarse_f32(t_row, g.random((n, s), dtype=np.float32))
    sigma = (g.random((n, s), dtype=np.float32) * 3).astype(np.float32)
    sigma[0] = 0.0
    if n > 1:
        sigma[1] *= 40.0
    c = g.random((n, s, 3), dtype=np.float32)
    up = (g.standard_normal((n, 3)).astype(np.float32), g.standard_normal(n).astype(np.float32), g.standard_normal((n, s)).astype(np.float32))
    return dict(o=o, d=d, t_row=t_row, t=t, sigma=sigma, c=c, up=up, bg=np.array([1.0, 0.5, 0.25], np.float32))


def _judge_forward(got, fw, rows=slice(None)):
    budget = R.integrate_budget(fw)
    for k in ('rgb', 'depth', 'alpha', 'weights'):
        R.judge(k, got[k], fw[k][rows], budget[k][rows])


# ------------------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize('s', S_LIST)
def test_sample_coarse_bit_for_bit(s):
    n_max = max(_n_list())
    sc = _scene(n_max, s, seed=s)
    u = np.random.default_rng(s).random((n_max, s), dtype=np.float32)
    want_t = R.sample_coarse_f32(sc['t_row'], u)
    for n in _n_list():
        t, pos = dev_sample_coarse(sc['o'][:n], sc['d'][:n], sc['t_row'], u[:n])
        assert np.array_equal(t, want_t[:n]) and np.array_equal(pos, R.positions_f32(sc['o'][:n], sc['d'][:n], want_t[:n])), n
        t, pos = dev_sample_coarse(sc['o'][:n], sc['d'][:n], sc['t_row'], None)
        assert np.array_equal(t, np.broadcast_to(sc['t_row'], (n, s))) and np.array_equal(pos, R.positions_f32(sc['o'][:n], sc['d'][:n], t)), n


# ------------------------------------------------------------------------------------------------------------ compositing
@pytest.mark.parametrize('s', S_LIST)
def test_composite_forward_and_backward_within_budgets(s):
    n_max = max(_n_list())
    sc = _scene(n_max, s, seed=100 + s)
    for fd, bg in ((1e10, sc['bg']), (0.05, None), (0.05, sc['bg']), (1e10, None)):
        fw = R.integrate_f64(sc['t'], sc['d'], sc['sigma'], sc['c'], bg, fd)
        d_sigma, d_c, bw = R.integrate_backward_f64(fw, *sc['up'])
        b_sigma, b_c = R.backward_budget(fw, bw)
        assert fw['alpha'][0] == 0.0 and fw['depth'][0] == 0.0
        for n in (_n_list() if bg is not None else [37]):
            cut = lambda a: a[:n]      # noqa: E731
            got = dev_forward(cut(sc['t']), cut(sc['d']), cut(sc['sigma']), cut(sc['c']), bg, fd)
            _judge_forward(got, fw, slice(0, n))
            assert got['alpha'][0] == 0.0 and got['depth'][0] == 0.0 and np.array_equal(got['rgb'][0], bg if bg is not None else np.zeros(3, np.float32))
            gs, gc = dev_backward([cut(x) for x in sc['up']], cut(sc['t']), cut(sc['d']), cut(sc['sigma']), cut(sc['c']), bg, fd)
            R.judge('d_sigma', gs, d_sigma[:n], b_sigma[:n])
            R.judge('d_rgb_samples', gc, d_c[:n], b_c[:n])


def test_composite_null_gradients_determinism_and_ray_independence():
    n, s = 37, 65
    sc = _scene(n, s, seed=7)
    args = (sc['t'], sc['d'], sc['sigma'], sc['c'], sc['bg'], 0.05)
    first, again = dev_forward(*args), dev_forward(*args)
    assert all(np.array_equal(first[k], again[k]) for k in first)
    b1, b2 = dev_backward(sc['up'], *args), dev_backward(sc['up'], *args)
    assert np.array_equal(b1[0], b2[0]) and np.array_equal(b1[1], b2[1])
    perm = np.random.default_rng(0).permutation(n)
    shuffled = dev_forward(sc['t'][perm], sc['d'][perm], sc['sigma'][perm], sc['c'][perm], sc['bg'], 0.05)
    assert all(np.array_equal(shuffled[k], first[k][perm]) for k in first)
    sb = dev_backward([x[perm] for x in sc['up']], sc['t'][perm], sc['d'][perm], sc['sigma'][perm], sc['c'][perm], sc['bg'], 0.05)
    assert np.array_equal(sb[0], b1[0][perm]) and np.array_equal(sb[1], b1[1][perm])
    zeros = [np.zeros_like(x) for x in sc['up']]
    for k in range(3):              # a null upstream gradient is a zero one
        with_null = [None if j == k else x for j, x in enumerate(sc['up'])]
        with_zero = [zeros[j] if j == k else x for j, x in enumerate(sc['up'])]
        a, b = dev_backward(with_null, *args), dev_backward(with_zero, *args)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
    a = dev_backward([None, None, None], *args)
    assert not a[0].any() and not a[1].any()


def test_composite_on_the_reference_fixtures(golden_dir):
    g = np.load(golden_dir / 'nerf_sampling.npz')
    for bg, rgb_name in ((g['bg'], 'rgb'), (None, 'rgb_nobg')):
        fw = R.integrate_f64(g['depth'], g['dirs'], g['dens'], g['cols'], bg, 1e10)
        got = dev_forward(g['depth'], g['dirs'], g['dens'], g['cols'], bg, 1e10)
        _judge_forward(got, fw)
        budget = R.integrate_budget(fw)         # ... and against what the reference itself computed, within the same budgets
        R.judge('rgb', got['rgb'], g[rgb_name], budget['rgb'])
        R.judge('weights', got['weights'], g['weights'], budget['weights'])
        R.judge('alpha', got['alpha'], g['alpha'][:, 0], budget['alpha'])
        R.judge('depth', got['depth'], g['depth_out'][:, 0], budget['depth'])
    z = np.load(golden_dir / 'composite_bw.npz')
    for tag in ('open', 'closed'):
        fd = float(z[f'{tag}_final_delta'])
        args = (z['depth'], z['dirs'], z[f'{tag}_dens'], z[f'{tag}_cols'], None, fd)
        fw = R.integrate_f64(*args)
        d_weights = (z[f'{tag}_gw'] + z[f'{tag}_gd'][:, None] * z['depth']).astype(np.float32)     # the depth-sum term enters through the weights
        up = (z[f'{tag}_gr'], z[f'{tag}_go'], d_weights)
        d_sigma, d_c, bw = R.integrate_backward_f64(fw, *up)
        b_sigma, b_c = R.backward_budget(fw, bw)
        _judge_forward(dev_forward(*args), fw)
        gs, gc = dev_backward(up, *args)
        R.judge('d_sigma', gs, d_sigma, b_sigma)
        R.judge('d_rgb_samples', gc, d_c, b_c)
        R.judge('d_sigma', gs, z[f'{tag}_d_dens'], b_sigma)             # ... and against the reference's own autograd, within the same budgets
        R.judge('d_rgb_samples', gc, z[f'{tag}_d_cols'], b_c)
        assert np.isfinite(gs).all()


# ------------------------------------------------------------------------------------------------------------ resampling
def _fine_scene(n, sc, seed):
    g = np.random.default_rng(seed)
    o, d = _rays(n, seed + 1)
    t_c = R.sample_coarse_f32(torch.linspace(2.0, 6.0, sc).numpy(), g.random((n, sc), dtype=np.float32))
    w = (g.random((n, sc), dtype=np.float32) ** 8).astype(np.float32)          # peaked, like compositing weights
    w[g.random((n, sc)) < 0.3] = 0.0
    w[0] = 0.0                                                                  # an empty ray: uniform pdf
    return o, d, t_c, w


def _check_fine(got, o, d, t_c, w, u):
    n, sc = t_c.shape
    cdf64 = R.cdf_f64(w)
    R.judge('cdf', got['cdf'], cdf64, R.cdf_bound(cdf64, sc) + 1e-300)
    assert np.all(np.diff(got['cdf'], axis=-1) >= 0)
    assert np.array_equal(got['t_fine'], R.fine_from_cdf_f32(t_c, got['cdf'], u))
    assert np.array_equal(got['t'], np.sort(np.concatenate((t_c, got['t_fine']), axis=-1), axis=-1))
    assert np.array_equal(got['positions'], R.positions_f32(o, d, got['t']))


@pytest.mark.parametrize('sc,sf', FINE_LIST)
def test_sample_fine_bit_for_bit(sc, sf):
    n_max = max(_n_list())
    o, d, t_c, w = _fine_scene(n_max, sc, seed=sc + sf)
    u_row = torch.linspace(0.0, 1.0, sf).numpy()
    u_rays = np.random.default_rng(sc).random((n_max, sf), dtype=np.float32)
    for n in _n_list():
        for u in (u_row, u_rays[:n]):
            _check_fine(dev_sample_fine(t_c[:n], w[:n], u, o[:n], d[:n]), o[:n], d[:n], t_c[:n], w[:n], u)
    if sc >= 8:
        assert np.allclose(dev_sample_fine(t_c[:1], w[:1], u_row, o[:1], d[:1])['cdf'][0], np.arange(sc - 1) / (sc - 2), rtol=0, atol=1e-4)   # the empty ray


def test_sample_fine_special_rays():
    sc = 16
    o, d = _rays(3, 4)
    t_c = np.broadcast_to(torch.linspace(2.0, 6.0, sc).numpy(), (3, sc)).copy()
    w = np.zeros((3, sc), np.float32)
    w[0, 5] = 100.0                                       # flat intervals everywhere but one: widths of about 1e-7 against the 1e-5 threshold
    w[2] = np.random.default_rng(1).random(sc, dtype=np.float32)
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    u = np.array([0.0, below_one, 1.0, 2.0, 0.25, 0.5, 5e-8, 3e-7], np.float32)
    got = dev_sample_fine(t_c, w, u, o, d)
    _check_fine(got, o, d, t_c, w, u)
    knots = R.knots_of(t_c)
    widths = np.diff(got['cdf'][0])
    assert widths[4] > 0.99 and np.all(np.delete(widths, 4) < 2e-7)
    assert np.all(got['t_fine'][:, 0] == knots[:, 0])                             # u = 0: the first knot
    assert np.all(got['t_fine'][:, 3] == knots[:, -1])                            # u above the last cdf value: the last knot
    assert np.all((got['t_fine'] >= knots[:, :1]) & (got['t_fine'] <= knots[:, -1:]))
    assert knots[0, 4] < got['t_fine'][0, 4] < got['t_fine'][0, 5] < knots[0, 5]   # inside the peak
    assert abs(float(got['t_fine'][0, 6]) - float(knots[0, 0])) < 1e-5             # inside a flat interval: its left knot + u (k1 - k0)
    # the cdf values themselves as u: upper_bound starts the next interval
    on = got['cdf'][:, 1:-1].copy()
    _check_fine(dev_sample_fine(t_c, w, on, o, d), o, d, t_c, w, on)


@pytest.mark.parametrize('name', ['fine', 'fine_rand'])
def test_sample_fine_on_the_reference_fixture(golden_dir, name):
    g = np.load(golden_dir / 'nerf_sampling.npz')
    u = torch.linspace(0.0, 1.0, 192).numpy() if name == 'fine' else g['fine_rand_u']
    o, d = _rays(37, 9)
    got = dev_sample_fine(g['depth'], g['weights'], u, o, g['dirs'])
    _check_fine(got, o, g['dirs'], g['depth'], g['weights'], u)
    bound, smallest = R.fine_depth_budget(g['depth'], g['weights'], u)
    assert smallest > 1.0e-5 + 4.0e-7
    R.judge(name, got['t_fine'], g[name], bound)


# ------------------------------------------------------------------------------------------------------------ the Python layer
def _torch_rays(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 1.3
    return o.to(DEV), d.to(DEV), torch.nn.functional.normalize(d, dim=-1).to(DEV)


def test_composite_under_autograd():
    sc = _scene(21, 65, seed=3)
    t, d, bg = _dev(sc['t']), _dev(sc['d']), _dev(sc['bg'])
    sigma, c = _dev(sc['sigma']).requires_grad_(), _dev(sc['c']).requires_grad_()
    rgb, depth, alpha, w = nerf.composite(t, d, sigma, c, bg, 0.05)
    assert rgb.shape == (21, 3) and depth.shape == alpha.shape == (21, 1) and w.shape == (21, 65) and not depth.requires_grad
    up = [_dev(x) for x in sc['up']]
    loss = (up[0] * rgb).sum() + (up[1] * alpha[:, 0]).sum() + (up[2] * w).sum()
    gs, gc = torch.autograd.grad(loss, (sigma, c))
    T = lambda a: torch.tensor(np.asarray(a, np.float64))    # noqa: E731
    s64, c64 = T(sc['sigma']).requires_grad_(), T(sc['c']).requires_grad_()
    r64, _, a64, w64 = nerf.integrate_samples(T(sc['t']), T(sc['d']), s64, c64, T(sc['bg']), 0.05)
    want = torch.autograd.grad((T(sc['up'][0]) * r64).sum() + (T(sc['up'][1]) * a64[:, 0]).sum() + (T(sc['up'][2]) * w64).sum(), (s64, c64))
    fw = R.integrate_f64(sc['t'], sc['d'], sc['sigma'], sc['c'], sc['bg'], 0.05)
    b_sigma, b_c = R.backward_budget(fw, R.integrate_backward_f64(fw, *sc['up'])[2])
    R.judge('d_sigma', gs.cpu().numpy(), want[0].numpy(), b_sigma + 1e-12 * np.abs(want[0].numpy()).max())
    R.judge('d_rgb', gc.cpu().numpy(), want[1].numpy(), b_c + 1e-14)
    # only rgb used: the other upstream gradients arrive as None
    rgb2 = nerf.composite(t, d, sigma, c, bg, 0.05)[0]
    only = torch.autograd.grad((up[0] * rgb2).sum(), sigma)[0]
    ref = dev_backward([sc['up'][0], None, None], sc['t'], sc['d'], sc['sigma'], sc['c'], sc['bg'], 0.05)[0]
    assert np.array_equal(only.cpu().numpy(), ref)


def _chain(coarse, fine, o, d, vd, bg, near, far, sc, sf, randomize, batch, query):
    """render_rays(device_rays=True) stage by stage through the public functions, judging each compositing against f64 on the very depths and network
    outputs the device used -> the outputs, concatenated like render_rays'"""
    out = {k: [] for k in ('rgb', 'alpha', 'depth', 'rgb_coarse', 'alpha_coarse', 'depth_coarse')}
    bgn = bg.cpu().numpy()

    def composite(t, dd, dens, col, tag):
        res = nerf.composite(t, dd, dens.reshape(t.shape), col.reshape(*t.shape, 3), bg)
        fw = R.integrate_f64(t.cpu().numpy(), dd.cpu().numpy(), dens.detach().cpu().numpy(), col.detach().cpu().numpy(), bgn, 1e10)
        _judge_forward({k: v.detach().cpu().numpy().reshape(fw[k].shape) for k, v in zip(('rgb', 'depth', 'alpha', 'weights'), res)}, fw)
        for k, v in zip(('rgb', 'depth', 'alpha'), res):
            out[k + tag].append(v)
        return res[3]
    for a in range(0, o.shape[0], batch):
        oo, dd, vv = o[a:a + batch], d[a:a + batch], vd[a:a + batch]
        if coarse is not None:
            t_c, pos = nerf.sample_coarse(oo, dd, sc, near, far, randomize)
            w_c = composite(t_c, dd, *query(coarse, pos, vv, sc), '_coarse')
            t, pos = nerf.sample_fine(t_c, w_c, sf, randomize, oo, dd)
        else:
            t, pos = nerf.sample_coarse(oo, dd, sf, near, far, randomize)
        composite(t, dd, *query(fine, pos, vv, t.shape[1]), '')
    return {k: torch.cat(v) for k, v in out.items() if v}


@pytest.mark.parametrize('mode', ['fused_train', 'torch'])
@pytest.mark.parametrize('randomize,with_coarse', [(True, True), (False, True), (True, False)])
def test_render_rays_device_rays(mode, randomize, with_coarse):
    torch.manual_seed(5)
    coarse, fine = nerf.NeRFBlock(2, 1, 128, 4, 2).to(DEV), nerf.NeRFBlock(2, 1, 128, 4, 2).to(DEV)
    with torch.no_grad():
        for b in (coarse, fine):
            b.density_layer.bias.fill_(0.5)
    o, d, vd = _torch_rays(37)
    bg = torch.tensor([1.0, 0.5, 0.25], device=DEV)
    sc, sf, batch = 16, 24, 16
    flags = dict(fused_train=True) if mode == 'fused_train' else {}
    kw = dict(ray_batch_size=batch, n_samples_coarse_nerf=sc, n_samples_nerf=sf, randomize_samples=randomize, **flags)

    def query(block, pos, vv, s):
        if mode == 'fused_train':
            return nerf.fused_apply(block, pos, vv, dir_group=s)
        return block(pos, vv[:, None, :].expand(-1, s, -1).reshape(-1, 3))
    torch.manual_seed(17)
    got = nerf.render_rays(coarse if with_coarse else None, fine, o, d, vd, 2.0, 6.0, bg, device_rays=True, **kw)
    torch.manual_seed(17)
    want = _chain(coarse if with_coarse else None, fine, o, d, vd, bg, 2.0, 6.0, sc, sf, randomize, batch, query)    # judged against f64 inside
    assert got.keys() == want.keys()
    for k in got:
        assert torch.equal(got[k], want[k]), k                # same seed, same kernels, fixed orders: the same bits
    sum(v.sum() for k, v in got.items() if 'depth' not in k).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fine.parameters())
    # the torch path with the same seed sees depths that differ in their last bits (lerp against lower + (upper - lower) u; another cdf summation order),
    # which the network turns into output differences far above the compositing's rounding: a wiring check at 2e-2 of the unit colour range, where a
    # wrong u order, a wrong block or unsorted depths would show as errors of order 0.1 .. 1.  The budgets were applied inside _chain.
    torch.manual_seed(17)
    with torch.no_grad():
        ref = nerf.render_rays(coarse if with_coarse else None, fine, o, d, vd, 2.0, 6.0, bg, **kw)
    for k in ('rgb', 'alpha') + (('rgb_coarse', 'alpha_coarse') if with_coarse else ()):
        assert (got[k].detach() - ref[k]).abs().max().item() < 2e-2, k


def test_every_fallback_returns_torchs_bits():
    sc = _scene(9, 16, seed=2)
    t, d, o, bg = _dev(sc['t']), _dev(sc['d']), _dev(sc['o']), _dev(sc['bg'])
    sigma, c = _dev(sc['sigma']), _dev(sc['c'])
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))    # noqa: E731
    ref = nerf.integrate_samples(t, d, sigma, c, bg)
    assert same(nerf.composite(t.cpu(), d.cpu(), sigma.cpu(), c.cpu(), bg.cpu()), nerf.integrate_samples(t.cpu(), d.cpu(), sigma.cpu(), c.cpu(), bg.cpu()))
    dbl = [x.double() for x in (t, d, sigma, c, bg)]
    assert same(nerf.composite(*dbl), nerf.integrate_samples(*dbl)) and nerf.composite(*dbl)[0].dtype == torch.float64
    t_g, d_g = t.clone().requires_grad_(), d.clone().requires_grad_()
    assert same(nerf.composite(t_g, d, sigma, c, bg), ref) and nerf.composite(t_g, d, sigma, c, bg)[0].requires_grad
    assert same(nerf.composite(t, d_g, sigma, c, bg), ref)
    big_t = torch.linspace(2.0, 6.0, 1025, device=DEV).expand(2, 1025)
    big = (big_t, d[:2], torch.rand(2, 1025, device=DEV), torch.rand(2, 1025, 3, device=DEV), bg)
    assert same(nerf.composite(*big), nerf.integrate_samples(*big))
    # non-contiguous input is made contiguous, not refused
    tt = torch.stack((t, t), dim=-1)[..., 0]
    assert not tt.is_contiguous() and same(nerf.composite(tt, d, sigma, c, bg), nerf.composite(t, d, sigma, c, bg))
    # sampling
    for dd in (d_g, d.double()):
        oo = o.to(dd.dtype)
        torch.manual_seed(1)
        got = nerf.sample_coarse(oo, dd, 16, 2.0, 6.0, True)
        torch.manual_seed(1)
        want = nerf.generate_samples(9, 16, 2.0, 6.0, True, dd.dtype, dd.device)
        assert torch.equal(got[0], want) and torch.equal(got[1], (oo[:, None, :] + dd[:, None, :] * want[:, :, None]).reshape(-1, 3))
    w = ref[3]
    for tc, n_fine in ((t_g, 24), (t, 1025), (t.double(), 24)):
        ww, oo, dd = w.to(tc.dtype), o.to(tc.dtype), d.to(tc.dtype)
        torch.manual_seed(1)
        got = nerf.sample_fine(tc, ww, n_fine, True, oo, dd)
        torch.manual_seed(1)
        want = torch.sort(torch.cat((tc, nerf.generate_samples_from_pdf(tc, ww, n_fine, True)), dim=-1), dim=-1).values
        assert torch.equal(got[0], want) and torch.equal(got[1], (oo[:, None, :] + dd[:, None, :] * want[:, :, None]).reshape(-1, 3))


def test_graph_capture_replays_the_eager_bits():
    torch.manual_seed(9)
    block = nerf.NeRFBlock(2, 1, 128, 4, 2).to(DEV)
    with torch.no_grad():
        block.density_layer.bias.fill_(0.5)
    o, d, vd = _torch_rays(37, seed=2)
    bg = torch.tensor([1.0, 0.5, 0.25], device=DEV)
    u = torch.rand(37, 24, generator=torch.Generator().manual_seed(3)).to(DEV)
    target = torch.rand(37, 3, generator=torch.Generator().manual_seed(4)).to(DEV)

    def step():
        for p in block.parameters():
            p.grad = None
        t, pos = nerf.sample_coarse(o, d, 24, 2.0, 6.0, True, u=u)
        sigma, rgb = nerf.fused_apply(block, pos, vd, dir_group=24, grad_scale=1024.0)
        out, _, alpha, w = nerf.composite(t, d, sigma.reshape(37, 24), rgb.reshape(37, 24, 3), bg)
        t2, _ = nerf.sample_fine(t, w, 8, False, o, d)
        ((out - target).square().mean() + alpha.mean() * 1e-2).backward()
        return out.detach(), t2
    step()
    eager_out, eager_t2 = (x.clone() for x in step())
    eager = [p.grad.clone() for p in block.parameters()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_out, cap_t2 = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap_out, eager_out) and torch.equal(cap_t2, eager_t2)
    assert all(torch.equal(p.grad, e) for p, e in zip(block.parameters(), eager))
