"""CPU tests of the NeRF ray stages' reference (tests/nerf_rays_ref.py), of the C ABI's argument checks (header group 19) and of the Python fallbacks.
The f64 statements are pinned on the fixtures recorded from the reference's own code (tests/golden/nerf_sampling.npz, composite_bw.npz), the backward's
closed form on torch f64 autograd through nerf.integrate_samples; every planted defect breaks a case with a known answer and exceeds a budget."""
import ctypes

import numpy as np
import pytest
import torch

from nerficg_amd import _lib, nerf
from tests import nerf_rays_ref as R

EXPORTS = ('nrc_nerf_rays_per_group', 'nrc_nerf_rays_supported', 'nrc_nerf_sample_coarse', 'nrc_nerf_integrate_forward', 'nrc_nerf_integrate_backward',
           'nrc_nerf_sample_fine')


@pytest.fixture(scope='module')
def sampling(golden_dir):
    return dict(np.load(golden_dir / 'nerf_sampling.npz'))


@pytest.fixture(scope='module')
def composite_bw(golden_dir):
    return dict(np.load(golden_dir / 'composite_bw.npz'))


def _bw_case(z, tag, background=None, mut=None):
    fd = float(z[f'{tag}_final_delta'])
    fw = R.integrate_f64(z['depth'], z['dirs'], z[f'{tag}_dens'], z[f'{tag}_cols'], background, fd, mut=mut)
    d_weights = z[f'{tag}_gw'].astype(np.float64) + z[f'{tag}_gd'].astype(np.float64)[:, None] * z['depth']     # the fixture's depth-sum term
    return fw, (z[f'{tag}_gr'], z[f'{tag}_go'], d_weights), fd


# ------------------------------------------------------------------------------------------------------------ the f64 statements on the fixtures
def test_coarse_sampling_matches_the_fixture(sampling):
    g = sampling
    t_row = g['depth'][0]
    assert np.array_equal(R.sample_coarse_f32(t_row, None, 37), g['depth'])
    want = R.sample_coarse_f64(t_row, g['depth_rand_u'])
    assert np.all(np.abs(want - g['depth_rand']) <= 4 * R.U * np.abs(want))          # lower + (upper - lower) u: four roundings at most
    assert np.array_equal(R.sample_coarse_f32(t_row, g['depth_rand_u']), g['depth_rand'])   # the reference's own f32 sequence


def test_integration_matches_the_fixture(sampling):
    g = sampling
    fw = R.integrate_f64(g['depth'], g['dirs'], g['dens'], g['cols'], g['bg'], 1e10)
    budget = R.integrate_budget(fw)
    for key, name in (('rgb', 'rgb'), ('depth', 'depth_out'), ('alpha', 'alpha'), ('weights', 'weights')):
        R.judge(key, g[name].reshape(fw[key].shape), fw[key], budget[key])
    nobg = R.integrate_f64(g['depth'], g['dirs'], g['dens'], g['cols'], None, 1e10)
    R.judge('rgb_nobg', g['rgb_nobg'], nobg['rgb'], R.integrate_budget(nobg)['rgb'])
    assert fw['alpha'][3] == 0.0 and fw['depth'][3] == 0.0 and np.array_equal(fw['rgb'][3], g['bg'].astype(np.float64))     # the empty ray


@pytest.mark.parametrize('name', ['fine', 'fine_rand'])
def test_resampling_matches_the_fixture(sampling, name):
    g = sampling
    u = torch.linspace(0.0, 1.0, 192).numpy() if name == 'fine' else g['fine_rand_u']      # the row the reference itself lays out
    bound, smallest = R.fine_depth_budget(g['depth'], g['weights'], u)
    assert smallest > 1.0e-5 + 4.0e-7            # no sample sits in a flat interval, so nothing is excluded
    t64, cdf64, _, _ = R.sample_fine_f64(g['depth'], g['weights'], u)
    R.judge(name, g[name], t64, bound)
    t_sorted, t32, cdf32 = R.sample_fine_f32(g['depth'], g['weights'], u)
    R.judge(name + ' f32', t32, g[name], bound)
    R.judge('cdf', cdf32, cdf64, R.cdf_bound(cdf64, 64) + 1e-300)
    assert np.all(np.diff(cdf32, axis=-1) >= 0) and np.all(np.diff(t_sorted, axis=-1) >= 0)


@pytest.mark.parametrize('tag', ['open', 'closed'])
def test_backward_matches_the_fixture(composite_bw, tag):
    z = composite_bw
    fw, up, _ = _bw_case(z, tag)
    budget = R.integrate_budget(fw)
    R.judge('weights', z[f'{tag}_weights'], fw['weights'], budget['weights'])
    R.judge('alpha', z[f'{tag}_alpha'][:, 0], fw['alpha'], budget['alpha'])
    R.judge('rgb', z[f'{tag}_rgb'], fw['rgb'], budget['rgb'])
    d_sigma, d_cols, bw = R.integrate_backward_f64(fw, *up)
    b_sigma, b_cols = R.backward_budget(fw, bw)
    R.judge('d_sigma', z[f'{tag}_d_dens'], d_sigma, b_sigma)
    R.judge('d_cols', z[f'{tag}_d_cols'], d_cols, b_cols)
    assert np.isfinite(d_sigma).all()


@pytest.mark.parametrize('tag', ['open', 'closed'])
def test_backward_formula_against_torch_f64_autograd(composite_bw, tag):
    z = composite_bw
    bg = np.array([0.3, 0.6, 0.9])
    fw, up, fd = _bw_case(z, tag, bg)
    T = lambda a: torch.tensor(np.asarray(a, np.float64))   # noqa: E731
    sigma, cols = T(z[f'{tag}_dens']).requires_grad_(), T(z[f'{tag}_cols']).requires_grad_()
    rgb, _, alpha, w = nerf.integrate_samples(T(z['depth']), T(z['dirs']), sigma, cols, T(bg), fd)
    loss = (T(up[0]) * rgb).sum() + (T(up[1]) * alpha[:, 0]).sum() + (T(up[2]) * w).sum()
    want_sigma, want_cols = torch.autograd.grad(loss, (sigma, cols))
    d_sigma, d_cols, _ = R.integrate_backward_f64(fw, *up)
    scale = np.abs(want_sigma.numpy()).max(axis=-1, keepdims=True) + 1e-300
    assert np.all(np.abs(d_sigma - want_sigma.numpy()) <= 1e-12 * scale)
    assert np.all(np.abs(d_cols - want_cols.numpy()) <= 1e-14)


# ------------------------------------------------------------------------------------------------------------ planted defects
def _exceeds(name, got, want, bound):
    with pytest.raises(AssertionError):
        R.judge(name, got, want, bound)


def test_defect_strata_off_by_one(sampling):
    t_row, u = np.array([0.0, 2.0, 4.0, 6.0], np.float32), np.full((1, 4), 0.5, np.float32)
    assert np.array_equal(R.sample_coarse_f32(t_row, u), [[0.5, 2.0, 4.0, 5.5]])
    assert not np.array_equal(R.sample_coarse_f32(t_row, u, mut='strata_off_by_one'), [[0.5, 2.0, 4.0, 5.5]])
    g = sampling
    bad = R.sample_coarse_f64(g['depth'][0], g['depth_rand_u'], mut='strata_off_by_one')
    want = R.sample_coarse_f64(g['depth'][0], g['depth_rand_u'])
    _exceeds('t', bad, want, 4 * R.U * np.abs(want))


def test_defect_final_delta_not_scaled(composite_bw):
    one = lambda mut: R.integrate_f64([[3.0]], [[0.0, 0.0, 2.0]], [[1.0]], [[[1.0, 1.0, 1.0]]], None, 0.5, mut=mut)   # noqa: E731
    assert abs(one(None)['alpha'][0] - (1.0 - np.exp(-1.0))) < 1e-15 and abs(one('final_delta_unscaled')['alpha'][0] - (1.0 - np.exp(-0.5))) < 1e-15
    fw, _, _ = _bw_case(composite_bw, 'open')
    bad, _, _ = _bw_case(composite_bw, 'open', mut='final_delta_unscaled')
    _exceeds('weights', bad['weights'], fw['weights'], R.integrate_budget(fw)['weights'])


def test_defect_background_weighted_by_alpha(sampling):
    g = sampling
    args = (g['depth'], g['dirs'], g['dens'], g['cols'], g['bg'], 0.05)
    fw, bad = R.integrate_f64(*args), R.integrate_f64(*args, mut='background_alpha')
    assert np.array_equal(fw['rgb'][3], g['bg'].astype(np.float64)) and np.array_equal(bad['rgb'][3], np.zeros(3))    # the empty ray shows the background
    _exceeds('rgb', bad['rgb'], fw['rgb'], R.integrate_budget(fw)['rgb'])


def test_defect_epsilon_on_all_masses(sampling):
    w = np.full((1, 4), 3.0, np.float32)
    assert np.array_equal(R.cdf_f32(w), [[0.0, 0.5, 1.0]]) and np.array_equal(R.cdf_f64(w), [[0.0, 0.5, 1.0]])
    assert np.array_equal(R.cdf_f32(w, mut='eps_all_masses'), [[0.0, 0.25, 0.5]])
    want = R.cdf_f64(sampling['weights'])
    _exceeds('cdf', R.cdf_f64(sampling['weights'], mut='eps_all_masses'), want, R.cdf_bound(want, 64) + 1e-300)


def _peaked_ray():
    """one inner weight of 100, all others 0: every other interval of the cdf is about 1e-7 wide (flat), the peak's is almost 1"""
    t_c = np.linspace(2.0, 6.0, 8, dtype=np.float32)[None, :]
    w = np.zeros((1, 8), np.float32)
    w[0, 3] = 100.0
    return t_c, w


def test_defect_lower_bound_and_flat_rule():
    t_c, w = _peaked_ray()
    cdf, knots = R.cdf_f32(w), R.knots_of(t_c)
    widths = np.diff(cdf[0])
    assert widths[2] > 0.99 and np.all(np.delete(widths, 2) < 2e-7) and np.all(np.delete(widths, 2) > 0)
    u = np.array([cdf[0, 1], cdf[0, 1] * np.float32(0.5)], np.float32)       # exactly on a cdf value behind a flat interval; inside a flat interval
    good = R.fine_from_cdf_f32(t_c, cdf, u)
    # on the cdf value: upper_bound starts the NEXT interval -> the knot itself.  Inside the flat interval: width becomes 1 -> the left knot + u (k1 - k0)
    assert good[0, 0] == knots[0, 1] and good[0, 1] == knots[0, 0] + u[1] * (knots[0, 1] - knots[0, 0])
    lower = R.fine_from_cdf_f32(t_c, cdf, u, mut='lower_bound')
    assert lower[0, 0] != good[0, 0] and abs(float(lower[0, 0]) - float(knots[0, 0])) < 1e-5      # falls back into the flat interval: its left knot
    noflat = R.fine_from_cdf_f32(t_c, cdf, u, mut='no_flat_rule')
    assert noflat[0, 1] != good[0, 1] and abs(float(noflat[0, 1]) - 0.5 * float(knots[0, 0] + knots[0, 1])) < 1e-5
    # the budget of the GPU test is equality with this restatement: both defects exceed it on a dense row of u as well
    dense = np.linspace(0.0, 1.0, 192, dtype=np.float32)
    want = R.fine_from_cdf_f32(t_c, cdf, dense)
    assert not np.array_equal(R.fine_from_cdf_f32(t_c, cdf, dense, mut='no_flat_rule'), want)
    on_values = cdf[0, 1:-1].copy()
    assert not np.array_equal(R.fine_from_cdf_f32(t_c, cdf, on_values, mut='lower_bound'), R.fine_from_cdf_f32(t_c, cdf, on_values))


@pytest.mark.parametrize('mut', ['suffix_inclusive', 'T_i'])
def test_defect_in_the_backward(composite_bw, mut):
    # two samples of opacity 1/2: T = (1, 1/2), w = (1/2, 1/4); with d_weights = (1, 1): d_sigma = len (T_{i+1} - sum_{j>i} w_j) = (1/4, 1/4)
    ln2 = float(np.log(2.0))
    fw = R.integrate_f64(np.array([[1.0, 2.0]]), [[0.0, 0.0, 1.0]], [[ln2, ln2]], np.zeros((1, 2, 3)), None, 1.0)
    good, _, _ = R.integrate_backward_f64(fw, None, None, np.ones((1, 2)))
    bad, _, _ = R.integrate_backward_f64(fw, None, None, np.ones((1, 2)), mut=mut)
    assert np.allclose(good, [[0.25, 0.25]], rtol=0, atol=1e-15) and not np.allclose(bad, [[0.25, 0.25]], rtol=0, atol=1e-3)
    fw, up, _ = _bw_case(composite_bw, 'open')
    want, _, bw = R.integrate_backward_f64(fw, *up)
    _exceeds('d_sigma', R.integrate_backward_f64(fw, *up, mut=mut)[0], want, R.backward_budget(fw, bw)[0])


# ------------------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_group_19_exports_and_limits():
    lib = _lib.load()
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 18
    protos = _lib.parse_header()
    for name in EXPORTS:
        assert name in protos and hasattr(lib, name), name
    assert lib.nrc_nerf_rays_per_group() in (1, 2, 4, 8, 16)
    ok = lib.nrc_nerf_rays_supported
    assert [ok(s, 0) for s in (0, 1, 64, 1024, 1025, -1)] == [0, 1, 1, 1, 0, 0]
    assert [ok(*p) for p in ((3, 1), (64, 192), (1024, 1024), (2, 1), (1025, 1), (3, 1025), (64, -1))] == [1, 1, 1, 0, 0, 0, 0]


def test_group_19_validates_before_it_launches():
    """Unsupported sample counts, negative counts, null and misaligned pointers are answered before any HIP call (this machine has no GPU)."""
    lib = _lib.load()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)
    coarse = lambda n, s, ptrs: lib.nrc_nerf_sample_coarse(*ptrs[:4], n, s, *ptrs[4:], None)                      # noqa: E731
    fwd = lambda n, s, ptrs: lib.nrc_nerf_integrate_forward(*ptrs[:5], 1e10, n, s, *ptrs[5:], None)                # noqa: E731
    bwd = lambda n, s, ptrs: lib.nrc_nerf_integrate_backward(*ptrs[:8], 1e10, n, s, *ptrs[8:], None)               # noqa: E731
    fine = lambda n, sc, sf, ptrs, stride=0: lib.nrc_nerf_sample_fine(*ptrs[:3], stride, *ptrs[3:5], n, sc, sf, *ptrs[5:], None)   # noqa: E731
    for call, n_ptrs in ((coarse, 6), (fwd, 9), (bwd, 10)):
        nul = [None] * n_ptrs
        assert call(0, 64, nul) == 0 and call(-1, 64, nul) == -1 and call(5, 64, nul) == -1
        assert call(0, 0, nul) == -3 and call(0, 1025, nul) == -3 and call(5, 1025, [p] * n_ptrs) == -3
        for k in range(n_ptrs):
            assert call(5, 64, [odd if j == k else p for j in range(n_ptrs)]) == -1, (call, k)
    nul = [None] * 9
    assert fine(0, 64, 192, nul) == 0 and fine(-1, 64, 192, nul) == -1 and fine(5, 64, 192, nul) == -1
    assert fine(0, 2, 1, nul) == -3 and fine(0, 1024, 1025, nul) == -3 and fine(0, 1025, 1, nul) == -3 and fine(5, 64, 0, [p] * 9) == -3
    assert fine(5, 64, 192, [p] * 9, stride=100) == -1          # a row stride between 0 and S_fine
    for k in range(9):
        assert fine(5, 64, 192, [odd if j == k else p for j in range(9)]) == -1, k
    # the optional pointers may be null, the required ones may not: each required one alone
    for k in (0, 1, 2, 4, 5):
        assert coarse(5, 64, [None if j == k else p for j in range(6)]) == -1, k
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        assert fwd(5, 64, [None if j == k else p for j in range(9)]) == -1, k
    for k in (3, 4, 5, 6, 8, 9):
        assert bwd(5, 64, [None if j == k else p for j in range(10)]) == -1, k
    for k in (0, 1, 2, 3, 4, 5, 6):
        assert fine(5, 64, 192, [None if j == k else p for j in range(9)]) == -1, k


# ------------------------------------------------------------------------------------------------------------ the Python fallbacks
def _rays(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 1.3
    return o, d, torch.nn.functional.normalize(d, dim=-1)


@pytest.mark.parametrize('randomize,with_coarse', [(False, True), (True, True), (True, False)])
def test_render_rays_device_rays_on_cpu_is_the_torch_path(randomize, with_coarse):
    torch.manual_seed(3)
    coarse, fine = nerf.NeRFBlock(2, 1, 32, 4, 2), nerf.NeRFBlock(2, 1, 32, 4, 2)
    o, d, vd = _rays(21)
    kw = dict(ray_batch_size=8, n_samples_coarse_nerf=8, n_samples_nerf=12, randomize_samples=randomize)
    out = {}
    for flag in (False, True):
        torch.manual_seed(11)
        out[flag] = nerf.render_rays(coarse if with_coarse else None, fine, o, d, vd, 2.0, 6.0, torch.tensor([1.0, 0.5, 0.25]), device_rays=flag, **kw)
    assert out[True].keys() == out[False].keys()
    for k in out[False]:
        assert torch.equal(out[True][k], out[False][k]), k
    loss = sum(v.sum() for v in out[True].values())
    loss.backward()                                              # torch's autograd all the way
    assert fine.density_layer.weight.grad is not None


def test_stage_functions_on_cpu_return_torchs_bits():
    o, d, _ = _rays(9, seed=5)
    torch.manual_seed(2)
    t, pos = nerf.sample_coarse(o, d, 16, 2.0, 6.0, True)
    torch.manual_seed(2)
    want = nerf.generate_samples(9, 16, 2.0, 6.0, True, torch.float32, o.device)
    assert torch.equal(t, want) and torch.equal(pos, (o[:, None, :] + d[:, None, :] * want[:, :, None]).reshape(-1, 3))
    g = torch.Generator().manual_seed(8)
    sigma, rgb = (torch.rand(9, 16, generator=g) * 3).requires_grad_(), torch.rand(9, 16, 3, generator=g).requires_grad_()
    bg = torch.tensor([0.1, 0.2, 0.3])
    got, ref = nerf.composite(t, d, sigma, rgb, bg, 0.05), nerf.integrate_samples(t, d, sigma, rgb, bg, 0.05)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert torch.autograd.grad(got[0].sum() + got[3].sum(), sigma)[0].shape == sigma.shape
    w = ref[3].detach()
    for rnd in (False, True):
        torch.manual_seed(4)
        t2, pos2 = nerf.sample_fine(t, w, 24, rnd, o, d)
        torch.manual_seed(4)
        t_f = nerf.generate_samples_from_pdf(t, w, 24, rnd)
        want2 = torch.sort(torch.cat((t, t_f), dim=-1), dim=-1).values
        assert torch.equal(t2, want2) and torch.equal(pos2, (o[:, None, :] + d[:, None, :] * want2[:, :, None]).reshape(-1, 3))
