"""GPU: per-Gaussian contribution statistics of a rendered 3DGS view (GaussianRasterizer.contributions; C ABI nrc_gs_contributions_band; kernel
k_gs_contributions in nerficg_amd/csrc/gs_contrib.hip) and the pruning entry point on top (accumulate_contributions, Gaussians.prune_by_contribution).

Reference and budgets: tests/gs_contrib_ref.py (derivation in its docstring; held against a brute-force pixel loop in tests/test_gs_contrib_ref_cpu.py), built on
the kernel's own saved state as tests/test_gpu_gs_features.py builds its reference.  Every element of weight_sum and weight_max is judged against its own budget
where its magnitude is positive and must be exactly zero elsewhere; hits must equal the reference integer for integer.  The budget tests print the worst
error / budget per statistic."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import gs_contrib_ref as CR
from tests import gs_features_ref as F
from tests import gs_grad_cases as GC
from tests import gs_grad_ref as R
from tests import scenes
from tests import test_gpu_gs_features as FT
from tests import test_gpu_gs_grad_budget as BT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = BT.T
BASE = 'partial-70x45-deg3'
CASES = ('partial-9x5', 'full-16x16', BASE, 'dense-plain', 'clamp-alpha-0.999', 'single-wide', 'partial-113x71-2000-deg2')
KEYS = ('weight_sum', 'weight_max', 'hits')


def _render(c, grad=False, features=None, **kw):
    """One forward call of a fresh GaussianRasterizer on a case (every case here is of the 'sh' form).  Returns (rasterizer, outputs, leaves)."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    assert c.form == 'sh'
    sc = c.sc
    leaf = lambda a: T(a).requires_grad_(grad)
    m3, m2 = leaf(sc['means3D']), torch.zeros(c.n, 3, device=DEV, requires_grad=grad)
    op, sh, s, q = leaf(sc['opacities']), leaf(sc['shs']), leaf(sc['scales']), leaf(sc['rotations'])
    leaves = dict(mean3D=m3, mean2D=m2, opacity=op, scale=s, rot=q, sh=sh)
    if features is not None:
        kw['features'] = features
    rast = GaussianRasterizer(BT._settings(c))
    with torch.enable_grad() if grad else torch.no_grad():
        out = rast(means3D=m3, means2D=m2, opacities=op[:, None], shs=sh, scales=s, rotations=q, **kw)
    return rast, out, leaves


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, BlendRef) from the kernel's own saved state; the named cases share tests/test_gpu_gs_features.py's, 'second-view' is the base scene from another pose."""
    if name != 'second-view':
        c, st, st64, blend = FT._built(name)
        return c, blend
    c = GC._case(name, pose=(1.2, 0.45, 2.8))
    st, _ = GC.forward(c)
    out, leaves, state, _ = FT._forward(c, None)
    BT._check_state(st, state)
    blend = R.BlendRef(R.promote(st, **BT._kernel_floats(st, state)), np.zeros(3))
    masked = int(blend.ambiguous.sum())
    assert masked <= 0.005 * c.w * c.h, f'{masked} of {c.w * c.h} pixels are ambiguous'
    return c, blend


@functools.lru_cache(maxsize=None)
def _ref(name, kind, rows=None):
    """(map handed to the kernel, ContribRef): once per (case, map kind, pixel rows), shared, never modified.  kind 'ones': m = 1 with the ambiguous pixels
    zeroed; 'map': a random non-negative map with exact zeros, ambiguous pixels zeroed.  rows = (y0, y1): the reference of those pixel rows only (a band)."""
    c, blend = _built(name)
    m = CR.participation(blend, None if kind == 'ones' else CR.random_map(blend, seed=len(name)))
    assert masked_share(blend) <= 0.005
    m_ref = m
    if rows is not None:
        m_ref = np.zeros_like(m)
        m_ref[rows[0]:rows[1]] = m[rows[0]:rows[1]]
    return m, CR.ContribRef(blend, m_ref)


def masked_share(blend):
    return float(blend.ambiguous.sum()) / (blend.W * blend.H)


def _judge(label, got, want, budget, A):
    worst, over, nonzero = R.judge(got, want, budget, A)
    print(f'{label}: worst err / budget {worst:.3f}, {over} of {int((A > 0).sum())} over budget, {nonzero} of {int((A == 0).sum())} A == 0 elements not zero')
    assert over == 0 and nonzero == 0, (label, worst, over, nonzero)


def _judge_all(label, got, ref):
    """weight_sum and weight_max against their budgets, hits exactly."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g['weight_sum'].dtype == g['weight_max'].dtype == np.float32 and g['hits'].dtype == np.int32
    _judge(f'{label} weight_sum', g['weight_sum'], ref.weight_sum, ref.B, ref.A)
    _judge(f'{label} weight_max', g['weight_max'], ref.weight_max, ref.B_max, ref.weight_max)
    wrong = int((g['hits'].astype(np.int64) != ref.hits).sum())
    print(f'{label} hits: {wrong} of {ref.hits.size} differ, {int((ref.hits > 0).sum())} Gaussians hit, {int(ref.hits.sum())} hits')
    assert wrong == 0


# ------------------------------------------------------------------------------------------------------------------------ 1. budgets
@pytest.mark.parametrize('kind', ['ones', 'map'])
@pytest.mark.parametrize('name', CASES)
def test_every_statistic_within_its_budget(name, kind):
    c, blend = _built(name)
    m, ref = _ref(name, kind)
    rast, out, _ = _render(c)
    got = rast.contributions(T(m))
    assert set(got) == set(KEYS) and all(v.shape == (c.n,) for v in got.values())
    assert (ref.hits > 0).any()
    if kind == 'map':
        assert (m == 0).sum() > blend.ambiguous.sum()
    if name == 'dense-plain':
        assert max(tl.ids.size for tl in blend.tiles) > 256                              # some pixel walks past the first batch
    _judge_all(f'{name} {kind}', got, ref)
    if kind == 'ones' and not blend.ambiguous.any():                                      # no map at all is the map of ones
        again = rast.contributions()
        assert torch.equal(again['hits'], got['hits']) and torch.equal(again['weight_max'], got['weight_max'])
        _judge(f'{name} no map weight_sum', again['weight_sum'].cpu().numpy(), ref.weight_sum, ref.B, ref.A)


# ------------------------------------------------------------------------------------------------------------------------ 2. exactness
def test_two_views_in_both_orders():
    (c1, _), (c2, _) = _built(BASE), _built('second-view')
    (m1, ref1), (m2, ref2) = _ref(BASE, 'map'), _ref('second-view', 'map')
    r1, r2 = _render(c1)[0], _render(c2)[0]
    ab = r2.contributions(T(m2), out=r1.contributions(T(m1)))
    ba = r1.contributions(T(m1), out=r2.contributions(T(m2)))
    assert torch.equal(ab['hits'], ba['hits']) and torch.equal(ab['weight_max'], ba['weight_max'])     # integer add and max commute
    assert np.array_equal(ab['hits'].cpu().numpy(), ref1.hits + ref2.hits)
    want, B, A = ref1.weight_sum + ref2.weight_sum, ref1.B + ref2.B, ref1.A + ref2.A
    for label, got in (('view 1 then 2', ab), ('view 2 then 1', ba)):
        _judge(f'{label} weight_sum', got['weight_sum'].cpu().numpy(), want, B, A)
        _judge(f'{label} weight_max', got['weight_max'].cpu().numpy(), np.maximum(ref1.weight_max, ref2.weight_max), np.maximum(ref1.B_max, ref2.B_max),
               np.maximum(ref1.weight_max, ref2.weight_max))
    assert ((ref1.hits > 0) & (ref2.hits > 0)).any() and ((ref1.hits > 0) != (ref2.hits > 0)).any()


def test_three_bands_add_up_to_the_frame():
    c, blend = _built(BASE)                               # 70 x 45: three tile rows, the last 13 pixel rows high
    m, ref = _ref(BASE, 'map')
    whole = _render(c)[0].contributions(T(m))
    acc, want, B, A = None, 0, 0, 0
    for band in ((0, 1), (1, 1), (2, 1)):
        rows = (min(c.h, 16 * band[0]), min(c.h, 16 * (band[0] + band[1])))
        rb = _ref(BASE, 'map', rows)[1]
        rast = _render(c, tile_rows=band)[0]
        _judge_all(f'band {band}', rast.contributions(T(m)), rb)
        acc = rast.contributions(T(m), out=acc)
        want, B, A = want + rb.weight_sum, B + rb.B, A + rb.A
    assert torch.equal(acc['hits'], whole['hits']) and torch.equal(acc['weight_max'], whole['weight_max'])
    np.testing.assert_allclose(want, ref.weight_sum, rtol=1e-12, atol=0)                     # the bands' float64 sums are the frame's
    _judge('three bands weight_sum', acc['weight_sum'].cpu().numpy(), want, B, A)
    diff = np.abs(acc['weight_sum'].cpu().numpy().astype(np.float64) - whole['weight_sum'].cpu().numpy())
    assert (diff <= B + ref.B).all()                                                       # each side within its own budget of the common reference


# ------------------------------------------------------------------------------------------------------------------------ 3. the shipped detour
def test_weight_sum_equals_the_gradient_of_a_ones_feature():
    """features = ones(P, 1), backward of the (1, H, W) map with m as its gradient: features.grad = sum_p m w -- the only way to this number without the pass.
    Both within their own budgets of the common reference; the contributions call sits between the training forward and its backward."""
    c, blend = _built(BASE)
    m, ref = _ref(BASE, 'map')
    fr = F.FeatureRef(blend, np.ones((c.n, 1), np.float32))
    sums = fr.sums(m[None])
    BF = F.budget(sums)[1]
    assert (np.abs(sums['SF'][:, 0] - ref.weight_sum) <= 1e-12 * ref.A).all()
    ones = torch.ones(c.n, 1, device=DEV, requires_grad=True)
    rast, out, _ = _render(c, grad=True, features=ones)
    got = rast.contributions(T(m))
    out[2].backward(T(m[None]))
    _judge('features.grad', ones.grad.cpu().numpy()[:, 0], sums['SF'][:, 0], BF[:, 0], sums['AF'][:, 0])
    _judge_all('beside a feature pass', got, ref)


# ------------------------------------------------------------------------------------------------------------------------ 4. edge cases
def test_no_gaussians():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    c = _built(BASE)[0]
    rast = GaussianRasterizer(BT._settings(c))
    z = lambda *s: torch.zeros(*s, device=DEV)
    with torch.no_grad():
        rast(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 16, 3), scales=z(0, 3), rotations=z(0, 4))
    got = rast.contributions()
    assert all(got[k].shape == (0,) for k in KEYS) and got['hits'].dtype == torch.int32
    assert rast.contributions(torch.ones(c.h, c.w, device=DEV), out=got) is got


def test_a_zero_map_leaves_the_buffers_untouched_and_clear_clears():
    c, blend = _built(BASE)
    m, ref = _ref(BASE, 'map')
    rast = _render(c)[0]
    gen = torch.Generator(device=DEV).manual_seed(3)
    out = dict(weight_sum=torch.randn(c.n, device=DEV, generator=gen), weight_max=torch.rand(c.n, device=DEV, generator=gen),
               hits=torch.randint(0, 1000, (c.n,), device=DEV, generator=gen, dtype=torch.int32))
    before = {k: v.clone() for k, v in out.items()}
    assert rast.contributions(torch.zeros(c.h, c.w, device=DEV), out=out) is out
    assert all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in KEYS)      # bit for bit
    # accumulation on top of what is there: integer add and max exactly
    rast.contributions(T(m), out=out)
    assert np.array_equal(out['hits'].cpu().numpy(), before['hits'].cpu().numpy() + ref.hits)
    fresh = rast.contributions(T(m))
    assert torch.equal(out['weight_max'], torch.maximum(before['weight_max'], fresh['weight_max']))
    untouched = torch.from_numpy(ref.hits == 0).to(DEV)
    assert untouched.any() and torch.equal(out['weight_sum'][untouched], before['weight_sum'][untouched])
    # clear=True: what is there does not count
    rast.contributions(T(m), out=out, clear=True)
    assert torch.equal(out['hits'], fresh['hits']) and torch.equal(out['weight_max'], fresh['weight_max'])
    _judge('after clear weight_sum', out['weight_sum'].cpu().numpy(), ref.weight_sum, ref.B, ref.A)
    # and without it the second call adds: twice the hits, the same maximum; the second call's global atomics round partial sums of up to 2 A instead of A,
    # one per tile: gamma(tiles) A on top of the two budgets
    rast.contributions(T(m), out=out)
    assert torch.equal(out['hits'], 2 * fresh['hits']) and torch.equal(out['weight_max'], fresh['weight_max'])
    _judge('added twice weight_sum', out['weight_sum'].cpu().numpy(), 2 * ref.weight_sum, 2 * ref.B + R.gamma(ref.tiles) * ref.A, ref.A)


@pytest.mark.parametrize('only', KEYS)
def test_outputs_selected_one_at_a_time(only):
    c, blend = _built(BASE)
    m, ref = _ref(BASE, 'map')
    rast = _render(c)[0]
    got = rast.contributions(T(m), **{k: k == only for k in KEYS})
    assert list(got) == [only]
    full = rast.contributions(T(m))
    if only == 'weight_sum':
        _judge('weight_sum alone', got[only].cpu().numpy(), ref.weight_sum, ref.B, ref.A)
    else:
        assert torch.equal(got[only], full[only]) and bool(got[only].any())


def test_misuse_raises():
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    c = _built(BASE)[0]
    with pytest.raises(RuntimeError, match='not rendered'):
        GaussianRasterizer(BT._settings(c)).contributions()
    rast = _render(c)[0]
    ok = torch.ones(c.h, c.w, device=DEV)
    for bad, what in ((ok[:-1], 'shape'), (ok.t(), 'shape'), (ok[None], 'shape'), (ok.double(), 'dtype'), (ok.cpu(), 'device'), (ok.cpu().numpy(), 'device')):
        with pytest.raises(RuntimeError, match=f'pixel_weights.*{what}'):
            rast.contributions(bad)
    good = rast.contributions(ok)
    for bad in ({k: v[:-1] for k, v in good.items()}, {k: v.cpu() for k, v in good.items()}, {k: v.float() for k, v in good.items()}, {'hits': good['hits']}, [good]):
        with pytest.raises(RuntimeError, match='out'):
            rast.contributions(ok, out=bad)
    with pytest.raises(RuntimeError, match='at least one'):
        rast.contributions(ok, weight_sum=False, weight_max=False, hits=False)
    assert rast.contributions(ok, out={'hits': good['hits'].clone()}, weight_sum=False, weight_max=False)['hits'].equal(2 * good['hits'])
    rast.release_state()
    with pytest.raises(RuntimeError, match='release_state'):
        rast.contributions(ok)


def test_the_call_changes_nothing_the_forward_or_the_backward_returns():
    """On a frame of ONE tile (full-16x16), where the blend backward's records are reproducible (tests/test_gpu_gs_features.py states why)."""
    c, blend = _built('full-16x16')
    m, ref = _ref('full-16x16', 'map')
    g = T(GC.pixel_gradients(c)[0])
    rast, out, leaves = _render(c, grad=True)
    out[0].backward(g)
    plain = BT._gradients_of(c, leaves)
    rast2, out2, leaves2 = _render(c, grad=True)
    got_training = rast2.contributions(T(m))                 # after a training forward, before its backward
    out2[0].backward(g)
    got = BT._gradients_of(c, leaves2)
    assert torch.equal(out2[0], out[0]) and torch.equal(out2[1], out[1])
    for k in plain:
        assert np.array_equal(got[k], plain[k]), k
    rast3, out3, _ = _render(c)                               # under no_grad
    got_inference = rast3.contributions(T(m))
    assert torch.equal(out3[0], out[0].detach())
    assert torch.equal(got_inference['hits'], got_training['hits']) and torch.equal(got_inference['weight_max'], got_training['weight_max'])
    _judge_all('after a training forward', got_training, ref)
    _judge_all('after a forward under no_grad', got_inference, ref)


# ------------------------------------------------------------------------------------------------------------------------ 5. pruning end to end
def _walled_model():
    """400 Gaussians seen from three neighbouring orbit poses: 300 around the origin, a wall of 20 large splats of opacity 0.8 behind them (five of them take a
    pixel's transmittance below the blend's 1e-4 stop) and a block of 80 behind the wall."""
    from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera
    W, H = 64, 48
    poses = [scenes.orbit_pose(theta, 0.3, 3.0) for theta in (0.4, 0.5, 0.6)]
    away = -poses[1][:3, 3] / np.linalg.norm(poses[1][:3, 3])                               # from the middle camera through the origin
    rng = np.random.default_rng(5)
    sc = scenes.gs_random_scene(300, seed=2, extent=0.4, log_scale_mean=math.log(0.05))
    wall = (1.2 * away[None] + rng.normal(size=(20, 3)) * 0.02).astype(np.float32)
    hidden = (2.2 * away[None] + rng.uniform(-0.2, 0.2, size=(80, 3))).astype(np.float32)
    pos = np.concatenate([sc['means3D'], wall, hidden])
    scales = np.concatenate([sc['scales'], np.full((20, 3), 3.0, np.float32), np.full((80, 3), 0.05, np.float32)])
    ident = np.tile(np.array([1, 0, 0, 0], np.float32), (100, 1))
    rot = np.concatenate([sc['rotations'], ident])
    opac = np.concatenate([sc['opacities'].clip(1e-4, 1 - 1e-4), np.full(20, 0.8, np.float32), np.full(80, 0.9, np.float32)])
    shs = np.concatenate([sc['shs'], np.tile(sc['shs'][:1], (100, 1, 1))])
    g = Gaussians(T(pos), torch.log(T(scales)), T(rot), torch.logit(T(opac))[:, None], T(shs[:, :1]), T(shs[:, 1:]))
    g.training_setup(training_cameras_extent=3.0)
    cam = PerspectiveCamera(W, H, 1.2 * W, 1.2 * W, background_color=torch.tensor([0.1, 0.2, 0.3], device=DEV))
    return g, cam, poses


def test_pruning_what_no_view_sees():
    from nerficg_amd.gaussian_splatting import accumulate_contributions, render_image_inference, render_image_training
    g, cam, poses = _walled_model()
    views = [(cam, p) for p in poses]
    render_image_training(g, cam, poses[0])['rgb'].mean().backward()                        # one optimizer step: the Adam moments exist
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)
    before = [render_image_inference(g, cam, p, to_chw=True)['rgb'].clone() for p in poses]
    stats = accumulate_contributions(g, views)
    assert stats['n_views'] == 3 and all(stats[k].shape == (400,) for k in KEYS)
    hits = stats['hits']
    assert not bool(hits[320:].any()), 'a Gaussian behind the wall was blended'
    assert bool((hits[:300] > 0).any()) and bool((hits[300:320] > 0).any())
    assert bool(((stats['weight_max'] > 0) == (hits > 0)).all()) and bool(((stats['weight_sum'] > 0) == (hits > 0)).all())
    unseen = hits == 0
    kept_rows = g.get_positions.detach()[~unseen].clone()
    out = g.prune_by_contribution(stats, min_hits=1)
    assert out == {'pruned': int(unseen.sum()), 'kept': 400 - int(unseen.sum())} and out['pruned'] >= 80
    assert torch.equal(g.get_positions.detach(), kept_rows)                                 # exactly the hits == 0 rows are gone
    for group in g.optimizer.param_groups:
        p = group['params'][0]
        assert p.shape[0] == out['kept'], group['name']
        state = g.optimizer.state[p]
        assert state['exp_avg'].shape == p.shape and state['exp_avg_sq'].shape == p.shape, group['name']
    assert g.densification_gradient_accum.shape[0] == g.n_observations.shape[0] == out['kept']
    after = [render_image_inference(g, cam, p, to_chw=True)['rgb'] for p in poses]
    diff = max(float((a - b).abs().max()) for a, b in zip(after, before))
    print('three views after pruning: largest difference', diff, '(gate 2e-5); identical:', all(torch.equal(a, b) for a, b in zip(after, before)))
    assert diff <= 2e-5
    with pytest.raises(ValueError, match='Gaussians'):
        g.prune_by_contribution(stats, min_hits=1)                                          # the statistics of the model before pruning
    # a map per view and a callable give the same statistics as each other
    maps = [torch.rand(cam.height, cam.width, device=DEV, generator=torch.Generator(device=DEV).manual_seed(i)) for i in range(3)]
    a = accumulate_contributions(g, views, maps)
    b = accumulate_contributions(g, views, lambda image, index: maps[index] * (image.shape == (3, cam.height, cam.width)))
    assert torch.equal(a['hits'], b['hits']) and torch.equal(a['weight_max'], b['weight_max'])
    torch.testing.assert_close(a['weight_sum'], b['weight_sum'], rtol=2e-3, atol=0)
    assert bool((a['hits'] > 0).all())                                                      # everything that is left is seen
