"""GPU: gradients with respect to sample positions, directions and rays (nerficg_amd/csrc/ngp_input_grad.hip and what stands on it).

  * the two kernels against the float64 restatement of tests/input_grad_ref.py, EVERY element within its own budget c u sum|addends| (derivation there);
  * the tinycudann drop-in's x.grad against the restatement applied to the oracle's d_in, with the tolerance tests/test_gpu_tcnn_parity.py uses for d_in itself;
  * the wiring of InstantNGPRenderer.render_rays(train_mode=True) / density_gradient;
  * behaviour: a camera translation recovered by gradient descent through render_rays.
"""
import numpy as np
import pytest
import torch

import oracle
from nerficg_amd import _lib
from tests import input_grad_ref as R
from tests import scenes

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
NET_D = {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': 'None', 'n_neurons': 64, 'n_hidden_layers': 1}
NET_C = {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': 'Sigmoid', 'n_neurons': 64, 'n_hidden_layers': 2}


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


_TABLES: dict = {}


def _table(n_levels, n_features, log2_t):
    """(cfg, (entries, F) f32 numpy of fp16 values, fp16 device tensor), made once per grid"""
    key = (n_levels, n_features, log2_t)
    if key not in _TABLES:
        cfg = R.grid_cfg(n_levels, n_features, log2_t)
        table = R.random_table(cfg, seed=100 + n_levels + n_features + log2_t)
        _TABLES[key] = (cfg, table, T(table, torch.float16))
    return _TABLES[key]


def _grid_inputs(cfg, m, pair_major, seed):
    """positions, the upstream gradient (M, L F) for the restatement, and the same in the layout handed to the kernel (rows of 32 floats, NaN behind the
    grid's columns: nothing reads them; or pair-major [L][M][2])"""
    width = cfg['n_levels'] * cfg['n_features']
    x, g = R.positions(m, seed), R.upstream(m, width, seed + 1)
    if pair_major:
        dev = T(g.reshape(m, cfg['n_levels'], 2).transpose(1, 0, 2))
    else:
        full = np.full((m, 32), np.nan, np.float32)
        full[:, :width] = g
        dev = T(full)
    return x, g, dev


def _run_grid(lib, x_dev, d_dev, table_dev, cfg, pair_major):
    m = x_dev.shape[0]
    out = torch.full((m, 3), float('nan'), device=DEV)   # every row must be written
    _lib.check(lib.nrc_grid_backward_input(_lib.ptr(x_dev), m, _lib.ptr(d_dev), int(pair_major), _lib.ptr(table_dev), cfg['n_levels'], cfg['n_features'],
                                           cfg['log2_hashmap_size'], cfg['base_resolution'], cfg['per_level_scale'], _lib.ptr(out), _lib.stream_of(out)),
               'grid_backward_input')
    return out


GRIDS = [pytest.param(16, 2, True, id='16x2-pair-major'), pytest.param(16, 2, False, id='16x2'), pytest.param(8, 4, False, id='8x4'),
         pytest.param(12, 2, False, id='12x2'), pytest.param(5, 4, False, id='5x4')]


@pytest.mark.parametrize('m', [1, 63, 64, 257, 1000])
@pytest.mark.parametrize('log2_t', [19, 14])   # 14: low levels are hashed already, dense and hashed levels meet inside one workgroup
@pytest.mark.parametrize('n_levels,n_features,pair_major', GRIDS)
def test_grid_kernel_every_element_within_its_budget(n_levels, n_features, pair_major, log2_t, m):
    lib = _lib.load()
    cfg, table, table_dev = _table(n_levels, n_features, log2_t)
    x, g, d_dev = _grid_inputs(cfg, m, pair_major, seed=7 * m + log2_t)
    got = _run_grid(lib, T(x), d_dev, table_dev, cfg, pair_major).cpu().numpy().astype(np.float64)
    want, mag = R.grid_input_grad(x, g, table, cfg)
    budget = R.GRID_C(n_features) * R.U * mag
    err = np.abs(got - want)
    live = mag > 0
    print(f'grid input grad {n_levels}x{n_features} pm={pair_major} T=2^{log2_t} M={m}: worst error / budget {float((err[live] / budget[live]).max()) if live.any() else 0.0:.3f}')
    assert np.all(np.isfinite(got))
    assert np.all(err <= budget), float((err[live] / budget[live]).max())
    zero_rows = np.arange(m) % 4 == 1
    assert np.all(got[zero_rows] == 0.0)
    assert m < 4 or np.all(np.abs(got[~zero_rows]).sum(1) > 0)


@pytest.mark.parametrize('n_levels,n_features,pair_major', [(16, 2, True), (16, 2, False), (8, 4, False)])
def test_grid_kernel_gives_the_same_bits_twice(n_levels, n_features, pair_major):
    lib = _lib.load()
    cfg, _, table_dev = _table(n_levels, n_features, 14)
    x, _, d_dev = _grid_inputs(cfg, 1000, pair_major, seed=3)
    x_dev = T(x)
    a, b = _run_grid(lib, x_dev, d_dev, table_dev, cfg, pair_major), _run_grid(lib, x_dev, d_dev, table_dev, cfg, pair_major)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def _sh_inputs(m, degree, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d01 = (d * 0.5 + 0.5).astype(np.float16)
    special = np.array([[0.0, 1.0, 0.5], [1.0, 0.0, 0.0], [0.5, 0.5, 0.5]], np.float16)   # axis directions, faces of the cube, d = 0
    d01[:min(m, 3)] = special[:min(m, 3)]
    ident = (rng.normal(size=(m, 16)) * 0.5).astype(np.float16)
    g = R.upstream(m, 32, seed + 1)
    g[:, degree * degree:16] = 0.0   # coefficients a degree < 4 does not have meet zero first-layer weights: their d_in is zero
    return d01, ident, g


@pytest.mark.parametrize('ld', [19, 24])
@pytest.mark.parametrize('degree', [1, 2, 3, 4])
@pytest.mark.parametrize('m', [1, 65, 1000])
def test_sh_kernel_every_element_within_its_budget(m, degree, ld):
    lib = _lib.load()
    d01, ident, g = _sh_inputs(m, degree, seed=11 * m + degree)
    row = np.full((m, ld), np.nan, np.float16)
    row[:, :3], row[:, 3:19] = d01, ident
    x_dev, g_dev = T(row), T(g)
    out = torch.full((m, 19), float('nan'), device=DEV)
    _lib.check(lib.nrc_sh_identity_backward_input(_lib.ptr(x_dev), ld, m, _lib.ptr(g_dev), _lib.ptr(out), _lib.stream_of(out)), 'sh_identity_backward_input')
    got = out.cpu().numpy()
    want, mag = R.sh_input_grad(d01.astype(np.float64), g[:, :16])
    budget = R.SH_C * R.U * mag
    err = np.abs(got[:, :3].astype(np.float64) - want)
    live = mag > 0
    print(f'SH input grad degree {degree} M={m} ld={ld}: worst error / budget {float((err[live] / budget[live]).max()) if live.any() else 0.0:.3f}')
    assert np.all(np.isfinite(got))
    assert np.all(err <= budget)
    assert np.array_equal(got[:, 3:], g[:, 16:])                  # identity columns: copies
    assert degree > 1 or np.all(got[:, :3] == 0.0)                 # degree 1 is a constant
    assert np.all(got[1::4] == 0.0)


# ---- the drop-in -------------------------------------------------------------------------------------------------------------------------------------------
def _half_np(t):
    return t.detach().float().cpu().numpy().astype(np.float16).astype(np.float32)


def _grid_net(n_levels=16, n_features=2, seed=7):
    import nerficg_amd.tinycudann as tcnn
    enc = {'otype': 'Grid', 'type': 'Hash', 'n_levels': n_levels, 'n_features_per_level': n_features, 'log2_hashmap_size': 19, 'base_resolution': 16,
           'per_level_scale': R.PLS, 'interpolation': 'Linear'}
    net = tcnn.NetworkWithInputEncoding(3, 16, enc, NET_D, seed=seed).to(DEV)
    with torch.no_grad():   # amplify the table so that the encoded features are O(0.1) (as tests/test_gpu_tcnn_parity.py does)
        gen = torch.Generator().manual_seed(3)
        net.params[net.n_mlp_params:] = ((torch.rand(net.params.numel() - net.n_mlp_params, generator=gen) * 2 - 1) * 0.5).to(DEV)
    return net


def test_grid_network_hands_back_the_position_gradient():
    """x.grad of NetworkWithInputEncoding (16 x 2 grid) against the restatement applied to the oracle's d_in (oracle_mlp_bw), with the tolerance
    tests/test_gpu_tcnn_parity.py:163-166 uses for d_in itself.  Before the input-gradient kernels existed x.grad was None."""
    net = _grid_net()
    m = 3000
    x = R.positions(m, seed=31)
    g_out = (np.random.default_rng(32).normal(size=(m, 16)) * 0.01).astype(np.float16)
    xt = T(x).requires_grad_(True)
    net(xt).backward(T(g_out))
    assert xt.grad is not None and xt.grad.dtype == torch.float32 and xt.grad.shape == (m, 3)
    p = _half_np(net.params)
    cfg = R.grid_cfg(16, 2)
    table = p[3072:].reshape(-1, 2)
    enc = oracle.grid_encode_fw(x, table, 16, 19, 16, R.PLS)
    ref_out, acts = oracle.mlp_fw(enc, p[:3072], n_hidden=1, out_act=0, want_acts=True)
    _, d_in = oracle.mlp_bw(enc, p[:3072], ref_out, acts, g_out.astype(np.float32) * 128.0, n_hidden=1, out_act=0)
    want, _ = R.grid_input_grad(x, d_in / 128.0, table, cfg)
    got = xt.grad.cpu().numpy()
    print(f'grid network x.grad: worst |error| {np.abs(got - want).max():.3e} of max |gradient| {np.abs(want).max():.3e}')
    np.testing.assert_allclose(got, want, rtol=2e-2, atol=2e-3 * np.abs(want).max())


@pytest.mark.parametrize('degree', [1, 2, 3, 4])
def test_composite_network_hands_back_the_direction_gradient(degree):
    """x.grad of the SH + identity network, degrees 1-4 (the kernels always evaluate degree 4; coefficients the configuration lacks meet zero weights), against
    the restatement applied to the oracle's d_in on the kernel-layout weights.  Before: zeros in the three direction columns."""
    import nerficg_amd.tinycudann as tcnn
    enc = {'otype': 'Composite', 'nested': [{'n_dims_to_encode': 3, 'otype': 'SphericalHarmonics', 'degree': degree}, {'otype': 'Identity'}]}
    net = tcnn.NetworkWithInputEncoding(19, 3, enc, NET_C, seed=11).to(DEV)
    assert net.direction_gradient is False
    net.direction_gradient = True
    m = 2000
    d01, ident, _ = _sh_inputs(m, 4, seed=40 + degree)
    x = torch.cat([T(d01), T(ident)], dim=-1).float().requires_grad_(True)
    g_out = (np.random.default_rng(41).normal(size=(m, 3)) * 0.01).astype(np.float16)
    net(x).backward(T(g_out))
    p = net._half_params().float().cpu().numpy()    # kernel layout: first layer (64, 32), columns of absent coefficients zero
    cin = np.concatenate([oracle.sh4_encode(d01.astype(np.float32)), ident.astype(np.float32)], 1)
    ref_out, acts = oracle.mlp_fw(cin, p, n_hidden=2, out_act=1, want_acts=True)
    g_pad = np.zeros((m, 16), np.float32)
    g_pad[:, :3] = g_out.astype(np.float32) * 128.0
    _, d_in = oracle.mlp_bw(cin, p, ref_out, acts, g_pad, n_hidden=2, out_act=1)
    d_in /= 128.0
    assert np.all(d_in[:, degree * degree:16] == 0.0)
    want, _ = R.sh_input_grad(d01.astype(np.float64), d_in[:, :16])
    got = x.grad.cpu().numpy()
    print(f'composite network degree {degree}: worst direction |error| {np.abs(got[:, :3] - want).max():.3e} of max |gradient| {np.abs(want).max():.3e}')
    np.testing.assert_allclose(got[:, :3], want, rtol=2e-2, atol=2e-3 * np.abs(want).max())
    assert degree == 1 or np.abs(got[:, :3]).max() > 0
    np.testing.assert_allclose(got[:, 3:], d_in[:, 16:], rtol=2e-2, atol=2e-3 * np.abs(d_in).max())
    # the keyword overrides the attribute; switched off, the direction columns are the zeros they have always been and the identity columns the same bits
    x_off = x.detach().clone().requires_grad_(True)
    net(x_off, direction_gradient=False).backward(T(g_out))
    assert torch.equal(x_off.grad[:, :3], torch.zeros_like(x_off.grad[:, :3])) and torch.equal(x_off.grad[:, 3:], x.grad[:, 3:])


@pytest.mark.parametrize('n_levels,n_features', [(16, 2), (8, 4)])
def test_parameter_gradients_do_not_depend_on_the_input_gradient(n_levels, n_features):
    """Parameter gradients with and without x.requires_grad are bit-identical; with the parameters detached params.grad stays None and x.grad is unchanged.
    64 samples: one wave per level adds to the table and one workgroup to the weights, so the f32 atomics of the parameter gradients have one order."""
    net = _grid_net(n_levels, n_features)
    x = T(R.positions(64, seed=50))
    g_out = T((np.random.default_rng(51).normal(size=(64, 16)) * 0.01).astype(np.float16))
    net.zero_grad()
    net(x).backward(g_out)
    plain = net.params.grad.clone()
    net.params.grad = None
    xa = x.clone().requires_grad_(True)
    net(xa).backward(g_out)
    assert torch.equal(net.params.grad, plain) and int((plain[net.n_mlp_params:] != 0).sum()) > 0
    net.params.grad = None
    xb = x.clone().requires_grad_(True)
    net(xb, detach_params=True).backward(g_out)
    assert net.params.grad is None
    assert torch.equal(xb.grad, xa.grad) and float(xa.grad.abs().max()) > 0


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sphere():
    """The analytic sphere of tests/test_gpu_convergence.py trained for 300 iterations of that test's loop: a density field with a surface, an occupancy grid
    that marches samples, colours that depend on the position."""
    from nerficg_amd.apex_optimizers import FusedAdam
    from nerficg_amd.instant_ngp import Camera, InstantNGPModel, InstantNGPRenderer
    from nerficg_amd.raygen import generate_rays
    from tests.test_gpu_convergence import analytic_view, orbit
    W = H = 100
    fx, fy, cx, cy = scenes.lego_intrinsics(W, H)
    cam = Camera(width=W, height=H, focal_x=fx, focal_y=fy, center_x=cx, center_y=cy, near_plane=0.2, far_plane=1000.0, background_color=torch.ones(3))
    origins, dirs, colours, alphas = [], [], [], []
    for p in orbit(24, 0):
        rays = generate_rays(W, H, fx, fy, cx, cy, p, device=DEV, want_direction=False)
        img, hit = analytic_view(W, H, p, fx, fy, cx, cy, bg=(0.0, 0.0, 0.0))
        origins.append(rays['origin']); dirs.append(rays['view_direction'])
        colours.append(torch.from_numpy(img * hit[..., None]).reshape(-1, 3).to(DEV)); alphas.append(torch.from_numpy(hit.astype(np.float32)).reshape(-1).to(DEV))
    origins, dirs, colours, alphas = torch.cat(origins), torch.cat(dirs), torch.cat(colours), torch.cat(alphas)
    model = InstantNGPModel(RANDOM_SEED=0, device=DEV)
    renderer = InstantNGPRenderer(model)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15, betas=(0.9, 0.99), adam_w_mode=False)
    scaler = torch.amp.GradScaler(init_scale=128.0, growth_interval=10 ** 9)
    torch.manual_seed(0)
    perm = torch.randperm(origins.shape[0], generator=torch.Generator().manual_seed(0)).to(DEV)
    batch = 4096
    for it in range(300):
        if it % 16 == 0:
            renderer.update_occupancy_grid(warmup=it < 256)
        ids = perm[(it * batch) % (perm.numel() - batch):][:batch]
        with torch.amp.autocast('cuda'):
            bg = torch.rand(3, device=DEV)
            out = renderer.render_rays(origins[ids], dirs[ids], cam, train_mode=True, custom_bg_color=bg)
            target = colours[ids] + (1 - alphas[ids])[:, None] * bg
            loss = torch.nn.functional.mse_loss(out['rgb'].float(), target) + 0.5e-6 * model.weight_decay_mlp()
        scaler.scale(loss).backward()
        scaler.step(opt); scaler.update(); opt.zero_grad()
    renderer.update_occupancy_grid(warmup=False)
    pose = orbit(4, 1)[0]   # a held-out view
    rays = generate_rays(W, H, fx, fy, cx, cy, pose, device=DEV, want_direction=False)
    gt, _ = analytic_view(W, H, pose, fx, fy, cx, cy)
    return dict(model=model, renderer=renderer, cam=cam, origin=rays['origin'].contiguous(), view_direction=rays['view_direction'].contiguous(),
                gt=torch.from_numpy(gt).reshape(-1, 3).to(DEV))


def test_render_rays_carries_sample_gradients_to_the_rays(sphere, monkeypatch):
    """origin.grad = per-ray sum of the marched positions' gradients, view_direction.grad = per-ray sum of t g_xyz + g_dirs (RayMarcher.backward over the
    rays_a segments), both against float64 sums of the hooked per-sample gradients, within f32 summation error."""
    import nerficg_amd.instant_ngp as ingp
    renderer, cam = sphere['renderer'], sphere['cam']
    rows = torch.arange(300, device=DEV) + 100 * 48    # three image rows through the sphere
    origin = sphere['origin'][rows].clone().requires_grad_(True)
    view = sphere['view_direction'][rows].clone().requires_grad_(True)
    seen = {}
    query, composite = renderer.query, ingp.composite_over_background

    def spy_query(xyzs, dirs):
        xyzs.register_hook(lambda g: seen.__setitem__('g_xyzs', g.detach().clone()))
        dirs.register_hook(lambda g: seen.__setitem__('g_dirs', g.detach().clone()))
        return query(xyzs, dirs)

    def spy_composite(sigmas, rgbs, deltas, ts, rays_a, *rest):
        seen['ts'], seen['rays_a'] = ts, rays_a
        return composite(sigmas, rgbs, deltas, ts, rays_a, *rest)
    monkeypatch.setattr(renderer, 'query', spy_query, raising=False)
    monkeypatch.setattr(ingp, 'composite_over_background', spy_composite)
    noise = torch.rand(300, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = renderer.render_rays(origin, view, cam, train_mode=True, noise=noise)
    weights = torch.rand(300, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
    ((out['rgb'] * weights).sum() + out['depth'].sum()).backward()
    g_x, g_d = seen['g_xyzs'].double().cpu().numpy(), seen['g_dirs'].double().cpu().numpy()
    ts, rays_a = seen['ts'].double().cpu().numpy(), seen['rays_a'].cpu().numpy()
    assert g_x.shape[0] == ts.shape[0] > 1000 and np.abs(g_x).max() > 0 and np.abs(g_d).max() > 0
    want_o, want_d, tol_o, tol_d = np.zeros((300, 3)), np.zeros((300, 3)), np.zeros((300, 3)), np.zeros((300, 3))
    for ray, start, count in rays_a:
        sl = slice(start, start + count)
        want_o[ray] = g_x[sl].sum(0)
        want_d[ray] = (ts[sl, None] * g_x[sl] + g_d[sl]).sum(0)
        tol_o[ray] = (count + 4) * R.U * np.abs(g_x[sl]).sum(0)
        tol_d[ray] = (count + 4) * R.U * (np.abs(ts[sl, None] * g_x[sl]) + np.abs(g_d[sl])).sum(0)
    assert np.all(np.abs(origin.grad.double().cpu().numpy() - want_o) <= tol_o)
    assert np.all(np.abs(view.grad.double().cpu().numpy() - want_d) <= tol_d)
    assert np.abs(want_o).max() > 0 and np.abs(want_d).max() > 0
    # rays that do not require grad take the unchanged path: same picture for the same jitter
    monkeypatch.undo()
    with torch.no_grad():
        plain = renderer.render_rays(origin.detach(), view.detach(), cam, train_mode=True, noise=noise)
    assert float((plain['rgb'] - out['rgb'].detach()).abs().max()) <= 4e-3   # (the fused query against the module-by-module one: fp16 colours, 2e-3 per sample)


def test_a_fixed_sample_capacity_is_refused_by_name(sphere):
    renderer, cam = sphere['renderer'], sphere['cam']
    origin = sphere['origin'][:64].clone().requires_grad_(True)
    renderer.sample_capacity = 1 << 16
    try:
        with pytest.raises(RuntimeError, match='sample_capacity'):
            renderer.render_rays(origin, sphere['view_direction'][:64], cam, train_mode=True)
    finally:
        renderer.sample_capacity = None


def test_density_gradient_equals_autograd_through_the_module(sphere):
    import nerficg_amd.VolumeRenderingV2 as vr
    model, renderer = sphere['model'], sphere['renderer']
    pts = (torch.rand(5000, 3, generator=torch.Generator().manual_seed(8)) * 0.8 - 0.4).to(DEV)
    model.zero_grad()
    for p in model.parameters():
        p.grad = None
    sigma, grad = renderer.density_gradient(pts)
    assert all(p.grad is None for p in model.parameters())      # parameters detached: no gradient is handed out
    assert sigma.dtype == grad.dtype == torch.float32 and sigma.shape == (5000,) and grad.shape == (5000, 3) and not grad.requires_grad
    assert torch.equal(sigma, renderer.density(pts)) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    # (a) bit for bit sigma * d(log sigma)/dx by autograd through the module with its parameters attached: the same kernels, the same d_in
    x = pts.clone().requires_grad_(True)
    h0 = model.encoding_xyz((x - model.xyz_min) / model.xyz_size)[:, 0].float()
    g_log, = torch.autograd.grad(h0.sum(), x)
    assert torch.equal(sigma, h0.detach().exp()) and torch.equal(grad, sigma[:, None] * g_log)
    # (b) autograd of the density itself (TruncExp) through the module.  Its backward rounds the upstream gradient sigma to fp16 behind the loss scale 128,
    # so it is finite only below sigma = 65504 / 128 and differs from (a) by the fp16 roundings of the backward chain (d_out, two layers: 2^-11 each on
    # every addend of 64-term sums): rows with 1e-4 < sigma < 64 agree within 2e-2 of the row's largest component, the tolerance of d_in itself
    # (tests/test_gpu_tcnn_parity.py)
    x2 = pts.clone().requires_grad_(True)
    s = vr.TruncExp.apply(model.encoding_xyz((x2 - model.xyz_min) / model.xyz_size)[:, 0].float())
    want, = torch.autograd.grad(s.sum(), x2)
    low = (sigma < 64.0) & (sigma > 1e-4)   # (128 sigma a normal fp16 number, with room for the first layer's gain)
    diff = (grad[low] - want[low]).abs().max(dim=1).values
    scale = want[low].abs().max(dim=1).values
    print(f'density_gradient: {int(low.sum())} of 5000 points with 1e-4 < sigma < 64,{int((~torch.isfinite(want).all(dim=1)).sum())} rows of the direct gradient non-finite, '
          f'worst row difference {float((diff / scale.clamp_min(1e-30)).max()):.2e} of the row maximum, sigma max {float(sigma.max()):.3e}')
    assert int(low.sum()) > 50 and bool(torch.isfinite(want[low]).all())
    assert bool((diff <= 2e-2 * scale + 1e-12).all())


OFFSET = 0.05


def test_a_camera_translation_is_recovered_through_render_rays(sphere):
    """A held-out view whose camera position is off by 0.05: a 3-vector translation optimised by torch.optim.Adam through render_rays(train_mode=True), 80 steps
    of 4096 rays, the model frozen.  The translation error must end below half the offset; measured on an MI355X: 0.0500 -> 0.0030 after 40 steps -> 0.0018
    after 80 (0.0027 -> 0.0014 in another run: the sphere's training adds with f32 atomics and differs from run to run), so the bar is twice 0.0018."""
    model, renderer, cam = sphere['model'], sphere['renderer'], sphere['cam']
    offset = torch.tensor([0.6, -0.48, 0.64], device=DEV) * OFFSET
    t = torch.zeros(3, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([t], lr=2e-3)
    gen = torch.Generator().manual_seed(9)
    flags = [p.requires_grad for p in model.parameters()]
    for p in model.parameters():
        p.requires_grad_(False)
        p.grad = None
    try:
        errors = [float((offset + t.detach()).norm())]
        for step in range(80):
            ids = torch.randperm(sphere['origin'].shape[0], generator=gen)[:4096].to(DEV)
            noise = torch.rand(4096, generator=gen).to(DEV)
            out = renderer.render_rays(sphere['origin'][ids] + offset + t, sphere['view_direction'][ids], cam, train_mode=True, noise=noise)
            loss = torch.nn.functional.mse_loss(out['rgb'], sphere['gt'][ids])
            opt.zero_grad()
            loss.backward()
            opt.step()
            errors.append(float((offset + t.detach()).norm()))
    finally:
        for p, f in zip(model.parameters(), flags):
            p.requires_grad_(f)
    assert all(p.grad is None for p in model.parameters())
    print(f'camera translation: error {errors[0]:.4f} -> {errors[40]:.4f} (40 steps) -> {errors[-1]:.4f} (80 steps), final loss {float(loss.detach()):.3e}')
    assert errors[-1] < errors[0]
    assert errors[-1] < min(0.0036, 0.5 * OFFSET), errors[-1]   # measured: 0.0018 (another run, another training of the sphere: 0.0014)
