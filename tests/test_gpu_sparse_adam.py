"""GPU: the visibility-masked Adam step -- FusedAdam.step(visibility=...) over nrc_adam_step_rows_multi (csrc/adam_rows.hip, C ABI group 24) -- against
tests/sparse_adam_ref.py, against the dense step (the arbiter at an all-visible mask, bit for bit), and end to end through Gaussians.optimizer_step(radii).

Shapes: the six model tensors (P,3) (P,1,3) (P,15,3) (P,1) (P,3) (P,4) in one call, P in {1, 5, 64, 257, 1000}: work items of four floats straddle rows of
different visibility at widths 1, 3 and 45, and every tensor ends in a partial work item; P = 100 003 spreads the per-tensor block offsets over many workgroups.
Gradients of invisible rows are NaN, +-inf and 1e38 throughout: such a row must keep its bits whatever the gradient holds."""
import numpy as np
import pytest
import torch

from nerficg_amd.apex_optimizers import FusedAdam
from tests import scenes
from tests import sparse_adam_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BETAS, EPS = (0.9, 0.99), 1e-15
SIZES = (1, 5, 64, 257, 1000)
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3)


def model_shapes(P):
    return [(P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4)]


def make_mask(name, P, rng):
    """The issue's ten masks.  The seven patterns come in rotating dtypes; the last three are one random pattern in each representation."""
    rows = np.arange(P)
    random20 = rng.random(P) < 0.2
    pattern = {'all invisible': np.zeros(P, bool), 'all visible': np.ones(P, bool), 'alternating': rows % 2 == 0, 'only row 0': rows == 0,
               'only last row': rows == P - 1, 'random 20 %': random20, 'runs 64 / 192': rows % 256 < 64,
               'as bool': random20, 'as uint8 0 / 2': random20, 'as int32 -/0/+': random20}[name]
    as_u8 = lambda: torch.from_numpy(pattern.astype(np.uint8) * 2)
    as_i32 = lambda: torch.from_numpy(np.where(pattern, rng.integers(1, 90, P), rng.integers(-5, 1, P)).astype(np.int32))
    as_bool = lambda: torch.from_numpy(pattern)
    maker = {'all invisible': as_i32, 'all visible': as_u8, 'alternating': as_bool, 'only row 0': as_i32, 'only last row': as_u8, 'random 20 %': as_bool,
             'runs 64 / 192': as_i32, 'as bool': as_bool, 'as uint8 0 / 2': as_u8, 'as int32 -/0/+': as_i32}[name]
    t = maker()
    assert np.array_equal(SR.row_mask(t.numpy()), pattern)
    return t.to(DEV), pattern


def make_optimizer(shapes, rng, lrs=LRS, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(rng.normal(size=s).astype(np.float32)).to(DEV)) for s in shapes]
    groups = [{'params': [p], 'lr': lrs[k % len(lrs)], 'name': f't{k}'} for k, p in enumerate(params)]
    return FusedAdam(groups, lr=0.0, betas=BETAS, eps=EPS, **kw), params


def gradients(shapes, rng, visible=None):
    """Heavy-tailed random gradients; rows that `visible` calls invisible hold NaN, +inf, -inf, 1e38 in turn."""
    out = []
    for s in shapes:
        g = (rng.normal(size=s) * np.exp(rng.normal(size=s) * 2)).astype(np.float32)
        if visible is not None:
            poison = np.array([np.nan, np.inf, -np.inf, 1e38], np.float32)
            inv = np.nonzero(~visible)[0]
            g[inv] = poison[inv % 4].reshape((-1,) + (1,) * (len(s) - 1))
        out.append(g)
    return out


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).to(DEV)


def snapshot(opt, params):
    """(p, m, v) per parameter as numpy (zeros for moments that do not exist yet)."""
    out = []
    for p in params:
        st = opt.state.get(p, {})
        m = st['exp_avg'].cpu().numpy() if 'exp_avg' in st else np.zeros(tuple(p.shape), np.float32)
        v = st['exp_avg_sq'].cpu().numpy() if 'exp_avg_sq' in st else np.zeros(tuple(p.shape), np.float32)
        out.append((p.detach().cpu().numpy().copy(), m.copy(), v.copy()))
    return out


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


SEQUENCES = {
    'bias correction, no decay': (dict(bias_correction=True, weight_decay=0.0, adam_w_mode=False), ('all invisible', 'all visible', 'alternating', 'only row 0')),
    'no bias correction, L2 decay': (dict(bias_correction=False, weight_decay=0.01, adam_w_mode=False), ('only last row', 'random 20 %', 'runs 64 / 192', 'as bool')),
    'bias correction, AdamW decay': (dict(bias_correction=True, weight_decay=0.01, adam_w_mode=True), ('as uint8 0 / 2', 'as int32 -/0/+', 'alternating', 'random 20 %')),
    'no bias correction, AdamW decay': (dict(bias_correction=False, weight_decay=0.01, adam_w_mode=True), ('runs 64 / 192', 'all visible', 'only last row', 'as int32 -/0/+')),
}


@pytest.mark.parametrize('P', SIZES)
@pytest.mark.parametrize('sequence', list(SEQUENCES))
def test_1_2_four_masked_steps_match_the_reference_and_spare_invisible_rows(P, sequence):
    """Assertions 1 and 2: per step, invisible rows of p, m, v keep their bits (poisoned gradients), visible rows match tests/sparse_adam_ref.py within the
    tolerances of tests/test_gpu_adam_parity.py; a different mask each step; every group['step'] == 4 afterwards (global count, also through an
    all-invisible step)."""
    kw, masks = SEQUENCES[sequence]
    rng = np.random.default_rng(1000 + P)
    shapes = model_shapes(P)
    opt, params = make_optimizer(shapes, rng, **kw)
    for step, name in enumerate(masks, start=1):
        mask, pattern = make_mask(name, P, rng)
        grads = gradients(shapes, rng, pattern)
        set_grads(params, grads)
        before = snapshot(opt, params)
        opt.step(visibility=mask)
        after = snapshot(opt, params)
        for k, (b, a, g) in enumerate(zip(before, after, grads)):     # each step is held against the reference's step from the state it started in
            want = SR.step_f32(b[0], g, b[1], b[2], pattern, step, LRS[k], BETAS, EPS, kw['weight_decay'], kw['adam_w_mode'], kw['bias_correction'])
            SR.compare(b, a, want, pattern, what=f'P={P} step {step} ({name}) tensor {k}')
    assert [g['step'] for g in opt.param_groups] == [4] * 6
    assert all(np.isfinite(x).all() for triple in snapshot(opt, params) for x in triple)


@pytest.mark.parametrize('P', SIZES + (100_003,))
@pytest.mark.parametrize('kw', [dict(bias_correction=True, weight_decay=0.0, adam_w_mode=False), dict(bias_correction=False, weight_decay=0.01, adam_w_mode=True)],
                         ids=['plain', 'adamw-nobc'])
def test_3_all_visible_equals_the_dense_step_bit_for_bit(P, kw):
    """The dense step() is the parent's code and the arbiter: two steps of a twin optimizer, p, m and v compared bit for bit.  At P = 100 003 a third step under a
    random 20 % mask is held against the reference as well (block offsets of the six tensors spread over ~1 500 workgroups)."""
    rng = np.random.default_rng(7)
    shapes = model_shapes(P)
    masked, mp = make_optimizer(shapes, rng, **kw)
    dense, dp = make_optimizer(shapes, rng, **kw)
    with torch.no_grad():
        for a, b in zip(dp, mp):
            a.copy_(b)
    for step, dtype in ((1, torch.int32), (2, torch.bool)):
        grads = gradients(shapes, rng)
        set_grads(mp, grads); set_grads(dp, grads)
        masked.step(visibility=torch.ones(P, dtype=dtype, device=DEV))
        dense.step()
        for k, (a, b) in enumerate(zip(snapshot(masked, mp), snapshot(dense, dp))):
            for name, x, y in zip('pmv', a, b):
                assert bits_equal(x, y), f'P={P} step {step} tensor {k} {name}: {int((x.view(np.int32) != y.view(np.int32)).sum())} elements differ'
    if P == 100_003:
        mask, pattern = make_mask('random 20 %', P, rng)
        grads = gradients(shapes, rng, pattern)
        set_grads(mp, grads)
        before = snapshot(masked, mp)
        masked.step(visibility=mask)
        for k, (b, a, g) in enumerate(zip(before, snapshot(masked, mp), grads)):
            want = SR.step_f32(b[0], g, b[1], b[2], pattern, 3, LRS[k], BETAS, EPS, kw['weight_decay'], kw['adam_w_mode'], kw['bias_correction'])
            SR.compare(b, a, want, pattern, what=f'P={P} tensor {k}')


@pytest.mark.parametrize('P', (5, 257))
def test_4_views_four_bytes_past_a_16_byte_boundary_give_the_same_results(P):
    """base[1:].view(P, w): parameter, gradient and both moments misaligned in turn (any one of them sends the tensor down the single-float path)."""
    shapes = [(P, 3), (P, 3), (P, 45), (P, 1), (P, 3), (P, 4)]
    rng = np.random.default_rng(11)
    aligned, ap = make_optimizer(shapes, rng)
    off = lambda t: torch.cat([t.new_zeros(1), t.detach().reshape(-1)])[1:].view(t.shape)
    views = [torch.nn.Parameter(off(p)) for p in ap]
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    shifted = FusedAdam([{'params': [p], 'lr': LRS[k]} for k, p in enumerate(views)], lr=0.0, betas=BETAS, eps=EPS)
    for step, name in enumerate(('all visible', 'random 20 %', 'alternating'), start=1):
        mask, pattern = make_mask(name, P, rng)
        grads = gradients(shapes, rng, pattern)
        set_grads(ap, grads); set_grads(views, grads)
        if step == 2:      # step 1: the parameter alone is misaligned (fresh moments are aligned); from step 2 on the gradient and the moments are as well
            for k, v in enumerate(views):
                v.grad = off(v.grad)
                st = shifted.state[v]
                st['exp_avg'], st['exp_avg_sq'] = off(st['exp_avg']), off(st['exp_avg_sq'])
        aligned.step(visibility=mask); shifted.step(visibility=mask)
        for k, (a, b) in enumerate(zip(snapshot(aligned, ap), snapshot(shifted, views))):
            for nm, x, y in zip('pmv', a, b):
                assert bits_equal(x, y), f'P={P} step {step} tensor {k} {nm}'


def test_5_fourteen_parameters_take_two_launches_and_are_all_stepped():
    P = 257
    shapes = [(P, 1 + (k % 5)) for k in range(14)]
    rng = np.random.default_rng(5)
    opt, params = make_optimizer(shapes, rng)
    mask, pattern = make_mask('alternating', P, rng)
    grads = gradients(shapes, rng, pattern)
    set_grads(params, grads)
    before = snapshot(opt, params)
    opt.step(visibility=mask)
    for k, (b, a, g) in enumerate(zip(before, snapshot(opt, params), grads)):
        want = SR.step_f32(b[0], g, b[1], b[2], pattern, 1, LRS[k % len(LRS)], BETAS, EPS, 0.0, True)
        SR.compare(b, a, want, pattern, what=f'tensor {k}')
        assert not bits_equal(a[0][pattern], b[0][pattern]), f'tensor {k} was not stepped'
    assert [g['step'] for g in opt.param_groups] == [1] * 14


def test_6_7_no_gradients_is_a_silent_no_op_and_versions_advance():
    P = 64
    shapes = model_shapes(P)
    rng = np.random.default_rng(6)
    opt, params = make_optimizer(shapes, rng)
    before = snapshot(opt, params)
    versions = [p._version for p in params]
    opt.step(visibility=torch.ones(P + 9, dtype=torch.float32, device=DEV))      # a stale mask after densification: wrong length, not even looked at
    assert [p._version for p in params] == versions and len(opt.state) == 0 and all('step' not in g for g in opt.param_groups)
    assert all(bits_equal(x, y) for a, b in zip(before, snapshot(opt, params)) for x, y in zip(a, b))
    mask, pattern = make_mask('random 20 %', P, rng)
    set_grads(params, gradients(shapes, rng, pattern))
    opt.step(visibility=mask)
    assert [p._version for p in params] == [v + 1 for v in versions]
    # a parameter without a gradient is left alone, the others are stepped
    params[2].grad = None
    versions = [p._version for p in params]
    opt.step(visibility=mask)
    assert [p._version - v for p, v in zip(params, versions)] == [1, 1, 0, 1, 1, 1]
    assert [g['step'] for g in opt.param_groups] == [2, 2, 1, 2, 2, 2]


ERRORS = ('float mask', 'mask on the host', 'wrong length', 'two-dimensional mask', 'capturable', 'grad_scale', 'found_inf', 'half parameter', 'host parameter',
          'non-contiguous parameter', 'non-contiguous gradient', 'other first dimension', 'fp16 compute copy', 'L2 slice')


@pytest.mark.parametrize('case', ERRORS)
def test_8_every_violation_raises_and_leaves_everything_as_it_was(case):
    """One good masked step first (so moments and counters exist), then the violation: parameters, moments, counters and versions as before."""
    P = 64
    shapes = model_shapes(P)
    rng = np.random.default_rng(8)
    opt, params = make_optimizer(shapes, rng, capturable=False)
    mask, pattern = make_mask('alternating', P, rng)
    set_grads(params, gradients(shapes, rng, pattern))
    opt.step(visibility=mask)
    set_grads(params, gradients(shapes, rng, pattern))
    bad_mask = mask
    if case == 'float mask':
        bad_mask = mask.float()
    elif case == 'mask on the host':
        bad_mask = mask.cpu()
    elif case == 'wrong length':
        bad_mask = torch.ones(P - 1, dtype=torch.bool, device=DEV)
    elif case == 'two-dimensional mask':
        bad_mask = mask[:, None]
    elif case == 'capturable':
        opt.capturable = True
    elif case == 'grad_scale':
        opt.grad_scale = torch.ones(1, device=DEV)
    elif case == 'found_inf':
        opt.found_inf = torch.zeros(1, device=DEV)
    elif case == 'half parameter':
        q = torch.nn.Parameter(torch.zeros(P, 2, dtype=torch.float16, device=DEV)); q.grad = torch.zeros_like(q)
        opt.add_param_group({'params': [q], 'name': 'half'})
    elif case == 'host parameter':
        q = torch.nn.Parameter(torch.zeros(P, 2)); q.grad = torch.zeros_like(q)
        opt.add_param_group({'params': [q], 'name': 'host'})
    elif case == 'non-contiguous parameter':
        q = torch.nn.Parameter(torch.zeros(2, P, device=DEV).t()); q.grad = torch.zeros(P, 2, device=DEV)
        assert not q.is_contiguous()
        opt.add_param_group({'params': [q], 'name': 'strided'})
    elif case == 'non-contiguous gradient':
        q = torch.nn.Parameter(torch.zeros(P, 2, device=DEV)); q.grad = torch.zeros(2, P, device=DEV).t()
        assert not q.grad.is_contiguous()
        opt.add_param_group({'params': [q], 'name': 'strided_grad'})
    elif case == 'other first dimension':
        q = torch.nn.Parameter(torch.zeros(P + 1, 2, device=DEV)); q.grad = torch.zeros_like(q)
        opt.add_param_group({'params': [q], 'name': 'longer'})
    elif case == 'fp16 compute copy':
        params[1]._nrc_half_owner = lambda: None
    elif case == 'L2 slice':
        opt.set_l2_slice(params[3], 8, 1e-3)
    everything = [p for g in opt.param_groups for p in g['params']]
    before = snapshot(opt, params)
    versions, steps, n_state = [p._version for p in everything], [g.get('step') for g in opt.param_groups], len(opt.state)
    with pytest.raises((RuntimeError, ValueError)) as e:
        opt.step(visibility=bad_mask)
    needle = {'float mask': 'dtype', 'mask on the host': 'device', 'wrong length': 'rows', 'two-dimensional mask': 'shape', 'capturable': 'capturable',
              'grad_scale': 'GradScaler', 'found_inf': 'GradScaler', 'half parameter': r'half.*float32', 'host parameter': r'host.*CUDA',
              'non-contiguous parameter': r'strided.*contiguous', 'non-contiguous gradient': r'strided_grad.*contiguous', 'other first dimension': r'longer.*rows',
              'fp16 compute copy': r't1.*fp16', 'L2 slice': r't3.*L2 slice'}[case]
    assert e.match(needle), str(e.value)
    torch.cuda.synchronize()
    assert [p._version for p in everything] == versions and [g.get('step') for g in opt.param_groups] == steps and len(opt.state) == n_state
    assert all(bits_equal(x, y) for a, b in zip(before, snapshot(opt, params)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 9: end to end
def _model(sc):
    from nerficg_amd.gaussian_splatting import Gaussians
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return Gaussians(T(sc['means3D']), torch.log(T(sc['scales'])), T(sc['rotations']), torch.logit(T(sc['opacities']).clamp(1e-4, 1 - 1e-4))[:, None].contiguous(),
                     T(sc['shs'][:, :1]), T(sc['shs'][:, 1:]))


ATTRS = ('_positions', '_features_dc', '_features_rest', '_opacities', '_scales', '_rotations')


def test_9_one_training_iteration_steps_exactly_the_gaussians_the_frame_saw():
    from nerficg_amd.gaussian_splatting import PerspectiveCamera, render_image_training, training_loss
    P, W, H = 2000, 96, 64
    sc = scenes.gs_random_scene(P, seed=3)
    g, twin = _model(sc), _model(sc)
    g.training_setup(training_cameras_extent=3.0, sparse_adam=True)
    twin.training_setup(training_cameras_extent=3.0)
    cam = PerspectiveCamera(W, H, 1.2 * W, 1.2 * W, background_color=torch.zeros(3, device=DEV))
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(0)).to(DEV)
    pose = lambda theta, radius: torch.from_numpy(np.asarray(scenes.orbit_pose(theta, 0.3, radius), dtype=np.float32)).to(DEV)
    with pytest.raises(RuntimeError, match='sparse_adam'):
        render_image_training(g, cam, pose(0.8, 1.0), fuse_rest_step=True)
    out = render_image_training(g, cam, pose(0.8, 1.0))       # a camera inside the cloud: what lies behind it is culled
    training_loss(out['rgb'], target).backward()
    radii = out['radii']
    seen = (radii > 0).cpu().numpy()
    assert 0 < seen.sum() < P, int(seen.sum())
    with pytest.raises(RuntimeError, match='sparse_adam'):
        g.optimizer_step()
    for a in ATTRS:                                            # the twin takes the dense step on the very same gradients (two backward passes differ in their atomics' order)
        getattr(twin, a).grad = getattr(g, a).grad.clone()
    params = [getattr(g, a) for a in ATTRS]
    before = snapshot(g.optimizer, params)
    g.optimizer_step(radii)
    twin.optimizer_step()
    after = snapshot(g.optimizer, params)
    dense = snapshot(twin.optimizer, [getattr(twin, a) for a in ATTRS])
    for a, b, x, d in zip(ATTRS, before, after, dense):
        for name, bb, xx, dd in zip('pmv', b, x, d):
            assert bits_equal(xx[~seen], bb[~seen]), f'{a} {name}: rows the frame did not see changed'
            assert bits_equal(xx[seen], dd[seen]), f'{a} {name}: visible rows differ from the dense first step'
        assert not bits_equal(x[0][seen], b[0][seen]), f'{a}: no visible row moved'
    assert [grp['step'] for grp in g.optimizer.param_groups] == [1] * 6
    for i in range(3):
        g.optimizer.zero_grad()
        out = render_image_training(g, cam, pose(2.0 + 1.3 * i, 1.0 + 0.8 * i))
        training_loss(out['rgb'], target).backward()
        g.optimizer_step(out['radii'])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(getattr(g, a)).all()) for a in ATTRS)
    assert all(bool(torch.isfinite(t).all()) for st in g.optimizer.state.values() for t in st.values())
