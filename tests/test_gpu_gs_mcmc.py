"""GPU: the 3DGS-MCMC kernels (csrc/gs_mcmc.hip, include/nerficg_hip.h group 16) against the f64 reference of tests/gs_mcmc_ref.py, and the life cycle
relocate -> add_new -> step -> noise on the analytic sphere.  Every assertion is deterministic: fixed seeds, no timing.

Tolerances and where they come from:
  * relocation: 1 f32 ulp around the f64 reference rounded to f32 -- the kernel evaluates in f64 (error 4e-13, five orders below half an ulp) and rounds
    once, so only a value that sits on a rounding boundary can differ, by one;
  * noise: the per-element budget of gs_mcmc_ref.noise_ref (derived there rounding by rounding; tests/test_gs_mcmc_ref_cpu.py shows that three wrong
    kernels exceed it on these very inputs);
  * generator: 1e-5 absolute on a normal: the radius sqrt(-2 ln u) is at most sqrt(48 ln 2) = 5.77 and carries a few f32 ulp of logf and sqrtf
    (< 5.77 * 4 * 2^-23 = 3e-6), the angle's sine / cosine are accurate to ~1e-6 absolute at most (sincospif of 2 u: no range reduction of 2 pi u), times
    the radius < 6e-6: together below 1e-5;
  * regulariser: 4 ulp on a gradient (the kernel adds in f64 and rounds once: expected 0 or 1), 1e-6 relative on the two f64-accumulated losses.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import gs_mcmc_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ulp_distance(a, b):
    """Distance of two f32 arrays in units in the last place (0 = the same bits; +0 and -0 coincide)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


# ---------------------------------------------------------------------------------------------------------------- relocation
MOMENT_ROWS = (3, 3, 3, 3, 45, 45, 1, 1, 3, 3, 4, 4)       # both Adam moments of positions, f_dc, f_rest, opacities, scales, rotations


def test_relocation_matches_the_f64_reference_to_one_ulp():
    from nerficg_amd.gaussian_splatting import _mcmc_relocation
    inp = ref.relocation_inputs()
    P = inp['count'].shape[0]
    assert P == 4099
    want = ref.relocation_ref(inp['logits'], inp['log_scales'], inp['count'])
    logits, log_scales, count = dev(inp['logits']), dev(inp['log_scales']), dev(inp['count'])
    moments = [torch.ones(P, r, device=DEV) for r in MOMENT_ROWS]
    o_out, s_out = torch.full((P,), -1.0, device=DEV), torch.full((P, 3), -1.0, device=DEV)
    _mcmc_relocation(logits, log_scales, count, moments, o_out, s_out)
    torch.cuda.synchronize()
    hit = inp['count'] > 0
    got_l, got_s = logits.cpu().numpy().reshape(-1), log_scales.cpu().numpy()
    d_l = ulp_distance(got_l, want['logit'].astype(np.float32))
    d_s = ulp_distance(got_s, want['log_scale'].astype(np.float32))
    d_o = ulp_distance(o_out.cpu().numpy()[hit], want['opacity'].astype(np.float32)[hit])
    d_a = ulp_distance(s_out.cpu().numpy()[hit], want['scale'].astype(np.float32)[hit])
    print(f'relocation, P = {P}: worst ulp distance logit {d_l.max()}, log-scale {d_s.max()}, opacity {d_o.max()}, scale {d_a.max()}; '
          f'rows off by one: {(d_l == 1).sum()} / {(d_s == 1).sum()} / {(d_o == 1).sum()} / {(d_a == 1).sum()}')
    assert d_l.max() <= 1 and d_s.max() <= 1 and d_o.max() <= 1 and d_a.max() <= 1
    # rows that were not drawn: the same bits, and no activated value written
    assert np.array_equal(got_l[~hit].view(np.int32), inp['logits'].reshape(-1)[~hit].view(np.int32))
    assert np.array_equal(got_s[~hit].view(np.int32), inp['log_scales'][~hit].view(np.int32))
    assert (o_out.cpu().numpy()[~hit] == -1.0).all() and (s_out.cpu().numpy()[~hit] == -1.0).all()
    # moments: zero exactly on the drawn rows
    for m in moments:
        m = m.cpu().numpy()
        assert not m[hit].any() and (m[~hit] == 1.0).all()
    # both ends of the clamp occur, and the kernel lands on them
    low, high = want['clamped'] == -1, want['clamped'] == 1
    assert low.sum() > 100 and high.sum() == 3
    assert (o_out.cpu().numpy()[low] == np.float32(0.005)).all() and (o_out.cpu().numpy()[high] == np.float32(1.0 - 2.0 ** -24)).all()
    # and the scale span of the inputs is the one asked for
    s_in = np.exp(inp['log_scales'].astype(np.float64))
    assert s_in.min() < 2e-4 and s_in.max() > 5.0


def test_relocation_without_moments_and_outputs():
    from nerficg_amd.gaussian_splatting import _mcmc_relocation
    inp = ref.relocation_inputs(257, seed=1)
    want = ref.relocation_ref(inp['logits'], inp['log_scales'], inp['count'])
    logits, log_scales = dev(inp['logits']), dev(inp['log_scales'])
    _mcmc_relocation(logits, log_scales, dev(inp['count']), [])
    assert ulp_distance(logits.cpu().numpy().reshape(-1), want['logit'].astype(np.float32)).max() <= 1
    assert ulp_distance(log_scales.cpu().numpy(), want['log_scale'].astype(np.float32)).max() <= 1


# ---------------------------------------------------------------------------------------------------------------- noise, caller's z
@functools.lru_cache(maxsize=None)
def noise_case(P):
    inp = ref.noise_inputs(P)
    x_ref, budget, gate = ref.noise_ref(inp['positions'], inp['rotations'], inp['log_scales'], inp['logits'], inp['z'], inp['lr'])
    return inp, x_ref, budget, gate


def run_noise(inp, **kw):
    from nerficg_amd.gaussian_splatting import mcmc_noise
    x = dev(inp['positions'])
    mcmc_noise(x, dev(inp['rotations']), dev(inp['log_scales']), dev(inp['logits']), inp['lr'], **kw)
    return x


@pytest.mark.parametrize('P', [1, 63, 1000])
def test_noise_with_the_callers_draw_sits_inside_the_budget(P):
    inp, x_ref, budget, gate = noise_case(P)
    got = run_noise(inp, z=dev(inp['z'])).cpu().numpy().astype(np.float64)
    ratio = np.abs(got - x_ref) / budget
    print(f'noise, P = {P}: worst error / budget = {ratio.max():.3f} (median {np.median(ratio):.3f})')
    assert (ratio <= 1.0).all(), ratio.max()
    o = 1.0 / (1.0 + np.exp(-inp['logits'].astype(np.float64).reshape(-1)))
    moved = np.abs(got - inp['positions'].astype(np.float64))
    closed = gate < 1e-30
    full = o <= 0.005 * (1 + 1e-6)
    if P >= 63:
        assert closed.sum() >= P // 9 and full.sum() >= P // 4
    assert (moved[closed] <= budget[closed]).all()                      # o near 1: the position does not move (by less than its budget)
    assert (gate[full] >= 0.49).all()                                   # o <= 0.005: the gate is open, the row gets the full step --
    step = np.abs(x_ref - inp['positions'].astype(np.float64))         # -- which the kernel takes (within the budget, checked above) and which is no rounding artefact
    assert (moved[full].max(axis=1) >= 0.5 * step[full].max(axis=1)).all() and (step[full].max(axis=1) > 100 * budget[full].max(axis=1)).all()


def test_noise_gives_a_row_the_same_bits_through_both_load_shapes():
    """16-byte words when every pointer is 16-byte aligned, single floats otherwise: tensors that start one row into an allocation take the second path."""
    from nerficg_amd.gaussian_splatting import mcmc_noise
    inp, *_ = noise_case(1000)
    aligned = run_noise(inp, z=dev(inp['z']))
    shifted = {k: torch.cat([torch.zeros_like(dev(v)[:1]), dev(v)])[1:] for k, v in inp.items() if k != 'lr'}
    assert shifted['positions'].data_ptr() % 16 != 0 and shifted['positions'].is_contiguous()
    mcmc_noise(shifted['positions'], shifted['rotations'], shifted['log_scales'], shifted['logits'], inp['lr'], z=shifted['z'])
    assert torch.equal(aligned.view(torch.int32), shifted['positions'].contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- noise, the kernel's generator
SEED, ITERATION = (5 << 32) | 1234, 77


def test_generator_draw_matches_philox_and_box_muller():
    inp, *_ = noise_case(1000)
    z_out = torch.empty(1000, 3, device=DEV)
    x = run_noise(inp, seed=SEED, iteration=ITERATION, z_out=z_out)
    want = ref.box_muller(ref.generator_words(SEED, ITERATION, np.arange(1000)))
    err = np.abs(z_out.cpu().numpy().astype(np.float64) - want).max()
    print(f'generator: worst |z - f64 Box-Muller| = {err:.2e}')
    assert err <= 1e-5
    # the positions are those of the z_in path fed with the draw, bit for bit
    fed = run_noise(inp, z=z_out)
    assert torch.equal(x.view(torch.int32), fed.view(torch.int32))
    # the same (seed, iteration) again: the same bits
    z_again = torch.empty_like(z_out)
    x_again = run_noise(inp, seed=SEED, iteration=ITERATION, z_out=z_again)
    assert torch.equal(x.view(torch.int32), x_again.view(torch.int32)) and torch.equal(z_out.view(torch.int32), z_again.view(torch.int32))


def test_generator_does_not_depend_on_how_the_rows_are_cut_into_launches():
    from nerficg_amd.gaussian_splatting import mcmc_noise
    inp, *_ = noise_case(1000)
    z_one = torch.empty(1000, 3, device=DEV)
    one = run_noise(inp, seed=SEED, iteration=ITERATION, z_out=z_one)
    t = {k: dev(v) for k, v in inp.items() if k != 'lr'}
    z_two = torch.empty(1000, 3, device=DEV)
    for a, b in ((0, 400), (400, 1000)):
        part = {k: v[a:b].clone() for k, v in t.items()}
        z_part = torch.empty(b - a, 3, device=DEV)
        mcmc_noise(part['positions'], part['rotations'], part['log_scales'], part['logits'], inp['lr'], seed=SEED, iteration=ITERATION, z_out=z_part, row_offset=a)
        t['positions'][a:b] = part['positions']
        z_two[a:b] = z_part
    assert torch.equal(z_one.view(torch.int32), z_two.view(torch.int32)) and torch.equal(one.view(torch.int32), t['positions'].view(torch.int32))
    # a row beyond 2^32: the counter's second word
    z_far = torch.empty(63, 3, device=DEV)
    inp63, *_ = noise_case(63)
    run_noise(inp63, seed=SEED, iteration=ITERATION, z_out=z_far, row_offset=2 ** 32 + 5)
    want = ref.box_muller(ref.generator_words(SEED, ITERATION, np.arange(63, dtype=np.uint64) + np.uint64(2 ** 32 + 5)))
    assert np.abs(z_far.cpu().numpy() - want).max() <= 1e-5


def test_generator_keyed_by_the_device_step_and_by_seed_and_iteration():
    inp, *_ = noise_case(1000)
    z_host, z_dev, z_it, z_seed = (torch.empty(1000, 3, device=DEV) for _ in range(4))
    host = run_noise(inp, seed=SEED, iteration=ITERATION, z_out=z_host)
    step = torch.tensor([ITERATION], dtype=torch.int32, device=DEV)
    lr_dev = torch.tensor([inp['lr']], dtype=torch.float32, device=DEV)
    inp_wrong_lr = dict(inp, lr=123.0)                                    # with lr_dev the host value is not read
    on_dev = run_noise(inp_wrong_lr, seed=SEED, iteration=ITERATION + 9, z_out=z_dev, device_step=step, lr_dev=lr_dev)
    assert torch.equal(z_host.view(torch.int32), z_dev.view(torch.int32)) and torch.equal(host.view(torch.int32), on_dev.view(torch.int32))
    run_noise(inp, seed=SEED, iteration=ITERATION + 1, z_out=z_it)
    run_noise(inp, seed=SEED + 1, iteration=ITERATION, z_out=z_seed)
    for other in (z_it, z_seed):
        differs = (other != z_host).any(dim=1).float().mean().item()
        assert differs > 0.99, differs


def test_generator_statistics():
    P = 65539
    inp = ref.noise_inputs(P, seed=3)
    z = torch.empty(P, 3, device=DEV)
    run_noise(inp, seed=42, iteration=3, z_out=z)
    z = z.cpu().numpy().astype(np.float64)
    mean, var = z.mean(axis=0), z.var(axis=0)
    print(f'generator, P = {P}: mean {mean}, variance {var}, max |z| {np.abs(z).max():.3f}')
    assert (np.abs(mean) <= 5.0 / math.sqrt(P)).all()
    assert (np.abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / P)).all()
    assert np.abs(z).max() <= 5.78


def test_inject_noise_keyed_by_a_capturable_optimizers_own_scalars():
    """Gaussians.inject_noise(None): generator and rate come from the device step counter and the device learning rate of the `positions` group -- the same
    bits as the host path given that step and that rate; a plain optimizer has no such scalars and is refused."""
    from nerficg_amd.gaussian_splatting import Gaussians
    gen = torch.Generator().manual_seed(5)
    pts = (torch.rand(500, 3, generator=gen) - 0.5).to(DEV)

    def model(capturable):
        g = Gaussians.from_point_cloud(pts, sh_degree=1)
        g.training_setup(capturable=capturable)
        g._opacities.data.fill_(-6.0)                                   # o = 0.0025: the gate is open
        for p in g._six():
            p.grad = torch.full_like(p, 1e-3)
        g.optimizer.step()
        return g

    g = model(True)
    group = next(gr for gr in g.optimizer.param_groups if gr['name'] == 'positions')
    assert torch.is_tensor(group['step']) and int(group['step'].item()) == 1
    start = g._positions.data.clone()
    z_dev, z_host = torch.empty(500, 3, device=DEV), torch.empty(500, 3, device=DEV)
    g.inject_noise(None, seed=3, z_out=z_dev)
    moved = g._positions.data.clone()
    assert not torch.equal(moved, start)
    g._positions.data.copy_(start)
    g.inject_noise(1, seed=3, z_out=z_host)
    assert torch.equal(z_dev.view(torch.int32), z_host.view(torch.int32)) and torch.equal(moved.view(torch.int32), g._positions.data.view(torch.int32))
    want = ref.box_muller(ref.generator_words(3, 1, np.arange(500)))
    assert np.abs(z_dev.cpu().numpy() - want).max() <= 1e-5
    for p in g._six():
        p.grad = torch.full_like(p, 1e-3)
    g.optimizer.step()                                                  # the counter advances on the device: another draw
    z_next = torch.empty(500, 3, device=DEV)
    g.inject_noise(None, seed=3, z_out=z_next)
    assert np.abs(z_next.cpu().numpy() - ref.box_muller(ref.generator_words(3, 2, np.arange(500)))).max() <= 1e-5
    with pytest.raises(RuntimeError, match='capturable'):
        model(False).inject_noise(None)


# ---------------------------------------------------------------------------------------------------------------- regulariser
@pytest.mark.parametrize('P', [1, 1000, 600001])          # one lane; several workgroups; more rows than the capped grid covers in one pass
def test_regulariser_gradients_and_losses(P):
    from nerficg_amd.gaussian_splatting import mcmc_regulariser_grads
    rng = np.random.default_rng(P)
    logits = rng.uniform(-12.0, 17.0, (P, 1)).astype(np.float32)
    log_scales = rng.uniform(np.log(1e-4), np.log(10.0), (P, 3)).astype(np.float32)
    g_o = (rng.standard_normal((P, 1)) * 1e-5 * (rng.random((P, 1)) < 0.7)).astype(np.float32)      # some incoming gradients are zero
    g_s = (rng.standard_normal((P, 3)) * 1e-6 * (rng.random((P, 3)) < 0.7)).astype(np.float32)
    d_o, d_s, loss_o, loss_s = ref.regulariser_ref(logits, log_scales, 0.01, 0.02)
    want_o = (g_o.astype(np.float64).reshape(-1) + d_o).astype(np.float32)
    want_s = (g_s.astype(np.float64) + d_s).astype(np.float32)
    runs = []
    for _ in range(2):
        grad_o, grad_s = dev(g_o), dev(g_s)
        losses = mcmc_regulariser_grads(dev(logits), dev(log_scales), grad_o, grad_s, 0.01, 0.02)
        runs.append((grad_o, grad_s, losses))
    grad_o, grad_s, losses = runs[0]
    worst = max(ulp_distance(grad_o.cpu().numpy().reshape(-1), want_o).max(), ulp_distance(grad_s.cpu().numpy(), want_s).max())
    got = losses.cpu().numpy().astype(np.float64)
    print(f'regulariser, P = {P}: worst gradient ulp distance {worst}, losses {got} against {loss_o:.9e}, {loss_s:.9e}')
    assert worst <= 4
    assert abs(got[0] - loss_o) <= 1e-6 * loss_o and abs(got[1] - loss_s) <= 1e-6 * loss_s
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- life cycle
RADIUS = 0.3


def analytic_view(width, height, c2w, fx, fy, cx, cy, bg=(1.0, 1.0, 1.0)):
    """(H, W, 3) f32 picture of an opaque sphere of radius 0.3 coloured 0.5 + 0.5 * normal in front of a white background, by a closed-form ray / sphere
    intersection (pixel centres at +0.5, x right, y down, z forward): the scene of tests/test_gpu_convergence.py, restated."""
    ys, xs = np.meshgrid(np.arange(height) + 0.5, np.arange(width) + 0.5, indexing='ij')
    local = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)
    R, o = np.asarray(c2w)[:3, :3], np.asarray(c2w)[:3, 3]
    d = local @ R.T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    b = d @ o
    disc = b * b - (o @ o - RADIUS ** 2)
    hit = disc > 0
    t = -b - np.sqrt(np.where(hit, disc, 0.0))
    hit &= t > 0
    n = (o + t[..., None] * d) / RADIUS
    return np.where(hit[..., None], 0.5 + 0.5 * n, np.asarray(bg)[None, None]).astype(np.float32)


def test_life_cycle_on_the_analytic_sphere():
    """The MCMC loop of INTEGRATION.md: backward, regularisers, every 40 iterations relocate + add_new (which drop the gradients: that step is skipped),
    optimizer step, noise.  o >= 0.005 after a round is asked of the f32 sigmoid of an f32 logit: the logit of 0.005 (5.29, spacing 2^-21) is stored to
    half a spacing, which moves o by up to 2.4e-7 relative, and the sigmoid adds an ulp or two -- together below 2^-20 relative, the slack used here."""
    from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera, render_image_training, training_loss
    W, H = 160, 120
    fx = fy = 1.1 * W
    cam = PerspectiveCamera(W, H, fx, fy, background_color=torch.ones(3, device=DEV))
    rng = np.random.default_rng(2)
    poses = [scenes.orbit_pose(float(rng.uniform(0, 2 * math.pi)), float(rng.uniform(-0.7, 0.9)), scenes.LEGO_RADIUS) for _ in range(24)]
    targets = [torch.from_numpy(analytic_view(W, H, p, fx, fy, W / 2, H / 2)).permute(2, 0, 1).contiguous().to(DEV) for p in poses]
    pts = (torch.rand(2000, 3, generator=torch.Generator().manual_seed(0)) - 0.5) * 0.8
    g = Gaussians.from_point_cloud(pts.to(DEV), sh_degree=3)
    g.training_setup(training_cameras_extent=scenes.LEGO_RADIUS)
    torch.manual_seed(0)
    cap, n_iters, every = 2600, 240, 40
    order = np.random.default_rng(0).permutation(n_iters) % len(poses)
    losses, sizes, relocated = [], [], 0
    for it in range(n_iters):
        g.update_learning_rate(it)
        k = int(order[it])
        out = render_image_training(g, cam, poses[k])
        loss = training_loss(out['rgb'], targets[k])
        loss.backward()
        reg = g.add_mcmc_regulariser_grads()
        losses.append(float(loss.detach()) + float(reg[0]) + float(reg[1]))
        if (it + 1) % every == 0:
            P = g.get_positions.shape[0]
            relocated += g.relocate()['n_relocated']
            added = g.add_new(cap)
            now = g.get_positions.shape[0]
            sizes.append(now)
            assert now == P + added == min(cap, int(1.05 * P)) <= cap
            assert float(g.get_opacities.detach().min()) >= 0.005 * (1.0 - 2.0 ** -20)
            for name, attr in g._GROUP_OF.items():
                p = getattr(g, attr)
                state = g.optimizer.state[p]
                assert p.shape[0] == now and state['exp_avg'].shape == p.shape and state['exp_avg_sq'].shape == p.shape
                assert p.grad is None or added == 0
            assert g.densification_gradient_accum.shape[0] == now and g.n_observations.shape[0] == now
        g.optimizer.step()
        g.optimizer.zero_grad()
        g.inject_noise(it)
    print(f'3DGS-MCMC life cycle: sizes {sizes}, {relocated} rows relocated, loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert sizes == [2100, 2205, 2315, 2430, 2551, 2600]
    for p in g._six():
        assert bool(torch.isfinite(p).all())
        for m in g.optimizer.state[p].values():
            if torch.is_tensor(m):
                assert bool(torch.isfinite(m.float()).all())
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
