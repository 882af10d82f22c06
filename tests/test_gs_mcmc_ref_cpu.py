"""CPU: the f64 reference of 3DGS-MCMC (tests/gs_mcmc_ref.py) checked on its own, the host logic of Gaussians.relocate / add_new on CPU tensors against a
plain restatement, and the C ABI of group 16 (exported, versioned, refusing bad arguments before any device call).

  * relocation (A): the two identities the formulas were derived from, by quadrature: N stacked copies composite to the old opacity at the centre, and the
    line integral of their composited opacity equals the old Gaussian's; the double sum against its collapsed form and against 60-digit decimals.
  * noise (B): the per-element budget cannot hide a wrong kernel -- three mutants of the reference exceed it on the GPU test's own inputs.
  * host logic (D): the three device steps (relocation arithmetic, row gather, row scatter) are replaced by restatements on CPU tensors; everything
    else -- which rows are dead, the draw's counts, which moments are cleared, the row copies, the growth schedule, the dropped gradients -- is the
    shipped code.
"""
import ctypes
import math
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

from nerficg_amd import _lib, adam_utils
from nerficg_amd import gaussian_splatting as gs
from tests import gs_mcmc_ref as ref

NRC_OK, NRC_ERR_INVALID = 0, -1
SYMBOLS = ('nrc_gs_mcmc_noise', 'nrc_gs_mcmc_relocation', 'nrc_gs_mcmc_regularise')


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('o,n', [(0.5, 3), (0.9, 7), (0.3, 50)])
def test_a_stacked_copies_keep_the_centre_opacity_and_the_line_integral(o, n):
    logit = math.log(o / (1.0 - o))
    o_ref, o_new, denom = ref.relocation_one(logit, n)
    assert abs(o_ref - o) <= 1e-15
    # at the centre: 1 - (1 - o_new)^N = o
    assert abs((1.0 - (1.0 - o_new) ** n) - o) <= 1e-12 * o
    # along a line through the centre: sum_i a (1 - a)^(i-1) with a = o_new exp(-x^2 / 2 sigma_new^2); the trapezoid rule on a smooth integrand that has
    # decayed to nothing at both ends converges faster than any power of the step
    sigma = 0.37
    sigma_new = o / denom * sigma
    dx = sigma_new / 4096.0                                                  # (the step itself, not a difference of two abscissae: that would cancel)
    x = np.arange(-40 * 4096, 40 * 4096 + 1) * dx
    a = o_new * np.exp(-x * x / (2.0 * sigma_new ** 2))
    integrand = np.zeros_like(x)
    t = np.ones_like(x)
    for _ in range(n):
        integrand += a * t
        t *= 1.0 - a
    integral = math.fsum(integrand) * dx
    assert abs(integral - sigma_new * math.sqrt(2.0 * math.pi) * denom) <= 1e-12 * integral      # the expansion that defines denom
    assert abs(integral - o * sigma * math.sqrt(2.0 * math.pi)) <= 1e-12 * integral              # = the old Gaussian's integral


def test_a_one_copy_is_the_identity_and_the_count_saturates_at_fifty():
    for o in (0.005, 0.1, 0.5, 0.99, 1.0 - 2.0 ** -24):
        o_ref, o_new, denom = ref.relocation_one(math.log(o / (1.0 - o)), 1)
        assert abs(o_new - o_ref) <= 2e-16 and abs(denom - o_ref) <= 2e-16
    assert list(ref.copies([0, 1, 48, 49, 50, 80, 10 ** 6])) == [1, 2, 49, 50, 50, 50, 50]
    logits = ref.logit32([0.3, 0.3, 0.3]).reshape(3, 1)
    out = ref.relocation_ref(logits, np.zeros((3, 3), np.float32), [49, 50, 80])
    assert out['logit'][0] == out['logit'][1] == out['logit'][2] and (out['log_scale'][0] == out['log_scale'][2]).all()
    untouched = ref.relocation_ref(logits, np.full((3, 3), -2.5, np.float32), [0, 0, 0])
    assert (untouched['logit'] == logits.reshape(-1).astype(np.float64)).all() and (untouched['log_scale'] == -2.5).all()


def _denom_decimal(o_new: Decimal, n: int) -> Decimal:
    return sum((Decimal(math.comb(i - 1, k)) * (-1) ** k / Decimal(k + 1).sqrt() * o_new ** (k + 1) for i in range(1, n + 1) for k in range(i)), Decimal(0))


@pytest.mark.parametrize('n', [2, 7, 50])
@pytest.mark.parametrize('o', [0.005, 0.3, 0.999, 1.0 - 2.0 ** -24])
def test_a_the_f64_sums_agree_with_60_digit_decimals(o, n):
    """f64 loses at most 4e-13 on the double sum (worst at o = 1 - 2^-24, N = 50, where sum |terms| / denom = 4e4); the collapsed sum the kernel evaluates
    (sum_{i=k+1..N} C(i-1, k) = C(N, k+1)) is the same number."""
    getcontext().prec = 60
    logit = float(ref.logit32(o))
    o64, o_new, denom = ref.relocation_one(logit, n)
    d_o = 1 / (1 + (-Decimal(logit)).exp())
    d_new = 1 - (1 - d_o) ** (Decimal(1) / Decimal(n))
    d_denom = _denom_decimal(d_new, n)
    assert abs(Decimal(o_new) - d_new) <= Decimal(1e-13) * d_new
    assert abs(Decimal(denom) - d_denom) <= Decimal(1e-12) * d_denom
    assert abs(Decimal(ref.denom_collapsed(o_new, n)) - d_denom) <= Decimal(1e-11) * d_denom
    assert abs(Decimal(o64 / denom) - d_o / d_denom) <= Decimal(1e-12) * (d_o / d_denom)


def test_a_the_relocation_inputs_hit_both_ends_of_the_clamp():
    inp = ref.relocation_inputs()
    out = ref.relocation_ref(inp['logits'], inp['log_scales'], inp['count'])
    assert (out['clamped'] == -1).sum() > 100 and (out['clamped'] == 1).sum() == 3 and (out['clamped'] == 0).sum() > 1000
    pairs = {(int(a), int(b)) for a, b in zip(np.arange(4096) % 8, np.arange(4096) % 7)}
    assert len(pairs) == 56


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('P', [63, 1000])
@pytest.mark.parametrize('mutant', ['scale', 'transpose', 'gate'])
def test_b_the_budget_cannot_hide_a_wrong_kernel(mutant, P):
    inp = ref.noise_inputs(P)
    args = (inp['positions'], inp['rotations'], inp['log_scales'], inp['logits'], inp['z'], inp['lr'])
    x_ref, budget, gate = ref.noise_ref(*args)
    x_mut, _, _ = ref.noise_ref(*args, mutant=mutant)
    open_rows = gate > 1e-3
    assert open_rows.sum() >= P // 3
    caught = (np.abs(x_mut - x_ref) > budget).any(axis=1)
    assert caught[open_rows].mean() >= 0.9, (mutant, caught[open_rows].mean())
    # and the budget is a small fraction of the step it judges (rows with an open gate)
    step = np.abs(x_ref - inp['positions'].astype(np.float64)).max(axis=1)
    assert np.median(budget.max(axis=1)[open_rows] / step[open_rows]) < 1e-3


def test_b_the_reference_itself_sits_inside_its_budget_in_f32_torch():
    """The published tensor expression evaluated in f32 differs from the f64 reference by rounding only -- a sanity check of noise_torch (the benchmark's
    comparison partner), with a budget widened by the expression's own longer chain (it squares R diag(s) by a matrix product: 8 x)."""
    inp = ref.noise_inputs(1000)
    t = {k: torch.from_numpy(v) for k, v in inp.items() if k != 'lr'}
    got = ref.noise_torch(t['positions'], t['rotations'], t['log_scales'], t['logits'], t['z'], inp['lr']).numpy().astype(np.float64)
    x_ref, budget, _ = ref.noise_ref(inp['positions'], inp['rotations'], inp['log_scales'], inp['logits'], inp['z'], inp['lr'])
    assert (np.abs(got - x_ref) <= 8.0 * budget).all()


def test_b_generator_layout():
    """Counter (index lo, index hi, iteration lo, iteration hi), key (seed lo, seed hi) on the pinned Philox; Box-Muller bounded by sqrt(48 ln 2)."""
    from tests import philox_ref
    idx = np.array([0, 1, 2 ** 32 + 5], dtype=np.uint64)
    w = ref.generator_words(seed=(7 << 32) | 3, iteration=(9 << 32) | 4, index=idx)
    for r, i in enumerate(idx):
        one = philox_ref.philox4x32_10((int(i) & 0xffffffff, int(i) >> 32, 4, 9), (3, 7))
        assert [int(x[r]) for x in w] == [int(x) for x in one]
    z = ref.box_muller([np.array([0], np.uint32), np.array([0], np.uint32), np.array([0xffffffff], np.uint32), np.array([0x80000000], np.uint32)])
    assert abs(z[0, 0] - math.sqrt(48 * math.log(2))) < 1e-12 and abs(z[0, 1]) < 1e-12 and z[0, 2] == 0.0      # ua = 2^-24, ub = 0; uc = 1


# ---------------------------------------------------------------------------------------------------------------- D
def _fake_relocation(opacity_logits, log_scales, counts, moments, opacity_out=None, scales_out=None):
    out = ref.relocation_ref(opacity_logits.numpy(), log_scales.numpy(), counts.numpy())
    hit = torch.from_numpy(counts.numpy() > 0)
    opacity_logits[hit] = torch.from_numpy(out['logit'].astype(np.float32))[hit][:, None]
    log_scales[hit] = torch.from_numpy(out['log_scale'].astype(np.float32))[hit]
    assert len(moments) <= 12
    for m in moments:
        m[hit] = 0.0


def _fake_gather_rows(tensors, src, n_out, kind=None, zero_new=None):
    outs = []
    for t_i, t in enumerate(tensors):
        o = t[src[:n_out].long()].clone()
        if kind is not None and zero_new is not None and zero_new[t_i]:
            o[kind[:n_out] != 0] = 0.0
        outs.append(o)
    return outs


def _fake_scatter_rows(rows, tensors, dst):
    assert dst.unique().numel() == dst.numel()
    for r, t in zip(rows, tensors):
        t[dst.long()] = r


@pytest.fixture
def cpu_hooks(monkeypatch):
    monkeypatch.setattr(gs, '_mcmc_relocation', _fake_relocation)
    monkeypatch.setattr(adam_utils, 'gather_rows', _fake_gather_rows)
    monkeypatch.setattr(adam_utils, 'scatter_rows', _fake_scatter_rows)


def _model(P=1000, dead_every=10, seed=0):
    g_ = torch.Generator().manual_seed(seed)
    o = 0.02 + 0.9 * torch.rand(P, generator=g_)
    if dead_every:
        o[::dead_every] = 0.001
    g = gs.Gaussians(torch.randn(P, 3, generator=g_), torch.randn(P, 3, generator=g_) - 3.0, torch.randn(P, 4, generator=g_),
                     torch.log(o / (1 - o)).reshape(P, 1), torch.randn(P, 1, 3, generator=g_), torch.randn(P, 15, 3, generator=g_))
    g.training_setup(optimizer_class=torch.optim.Adam)
    for p in g._six():
        p.grad = torch.randn(p.shape, generator=g_)
    g.optimizer.step()                       # creates both moments of all six groups, non-zero
    return g


def _snapshot(g):
    model = {name: getattr(g, attr).detach().numpy().copy() for name, attr in g._GROUP_OF.items()}
    for m in ('exp_avg', 'exp_avg_sq'):
        model[m] = {name: g.optimizer.state[getattr(g, attr)][m].numpy().copy() for name, attr in g._GROUP_OF.items()}
    return model


def _assert_equal(g, model):
    for name, attr in g._GROUP_OF.items():
        assert np.array_equal(getattr(g, attr).detach().numpy(), model[name]), name
        for m in ('exp_avg', 'exp_avg_sq'):
            assert np.array_equal(g.optimizer.state[getattr(g, attr)][m].numpy(), model[m][name]), (name, m)


def test_d_relocate_matches_the_plain_restatement(cpu_hooks):
    g = _model()
    model = _snapshot(g)
    before = _snapshot(g)
    dead = np.arange(0, 1000, 10)
    alive = np.setdiff1d(np.arange(1000), dead)
    drawn = np.random.default_rng(0).choice(alive[:40], size=dead.size)        # few targets: counts up to several
    got = g.relocate(sampled=torch.from_numpy(drawn))
    dead_plain, moved = ref.relocate_plain(model, drawn)
    assert moved and np.array_equal(dead_plain, dead) and got == {'n_dead': 100, 'n_relocated': 100}
    _assert_equal(g, model)
    hit = np.unique(drawn)
    assert np.bincount(drawn).max() >= 3
    for name, attr in g._GROUP_OF.items():
        p = getattr(g, attr)
        assert p.grad is None                                                  # a row moved: this iteration's step is skipped
        for m in ('exp_avg', 'exp_avg_sq'):
            now = g.optimizer.state[p][m].numpy()
            assert not now[hit].any()                                          # drawn rows lose their moments
            assert np.array_equal(now[dead], before[m][name][dead]) and now[dead].any()      # dead rows keep theirs, as published
        assert np.array_equal(p.detach().numpy()[dead], p.detach().numpy()[drawn])           # the copy carries the new opacity and scale
    rest = np.setdiff1d(alive, hit)
    assert np.array_equal(g._opacities.detach().numpy()[rest], before['opacities'][rest])
    assert not np.array_equal(g._scales.detach().numpy()[hit], before['scales'][hit])
    assert g.densification_gradient_accum.shape == (1000, 1) and g.n_observations.shape == (1000, 1)


def test_d_relocate_without_dead_rows_changes_nothing(cpu_hooks):
    g = _model(dead_every=0)
    before = _snapshot(g)
    grads = [p.grad for p in g._six()]
    assert g.relocate() == {'n_dead': 0, 'n_relocated': 0}
    _assert_equal(g, before)
    assert all(p.grad is q for p, q in zip(g._six(), grads))                   # nothing moved: the gradients stay


def test_d_relocate_draws_live_rows_by_opacity(cpu_hooks):
    g = _model()
    torch.manual_seed(0)
    before = _snapshot(g)
    assert g.relocate() == {'n_dead': 100, 'n_relocated': 100}
    o = torch.sigmoid(g._opacities.detach()).reshape(-1)
    assert float(o.min()) >= 0.005 * (1 - 2.0 ** -20)
    dead = np.arange(0, 1000, 10)
    pos, old = g._positions.detach().numpy(), before['positions']
    for j in dead:                                                             # every dead row now sits on a row that was alive
        src = np.nonzero((old == pos[j]).all(axis=1))[0]
        assert src.size == 1 and src[0] % 10 != 0
    with pytest.raises(RuntimeError, match='live rows'):
        _model().relocate(sampled=torch.zeros(100, dtype=torch.int64))         # row 0 is dead


def test_d_growth_follows_the_cap(cpu_hooks):
    g = _model(dead_every=0)
    torch.manual_seed(1)
    sizes = []
    for _ in range(7):
        P = g._positions.shape[0]
        for p in g._six():
            p.grad = torch.zeros_like(p)
        n = g.add_new(1300)
        assert n == ref.growth(P, 1300)
        sizes.append(g._positions.shape[0])
        for p in g._six():
            assert p.shape[0] == sizes[-1] and (p.grad is None) == (n > 0)     # .grad is dropped only when rows were added
            st = g.optimizer.state[p]
            assert st['exp_avg'].shape == p.shape and st['exp_avg_sq'].shape == p.shape
        for group in g.optimizer.param_groups:
            assert group['params'][0] is getattr(g, g._GROUP_OF[group['name']])
        assert g.densification_gradient_accum.shape == (sizes[-1], 1) and g.n_observations.shape == (sizes[-1], 1)
    assert sizes == [1050, 1102, 1157, 1214, 1274, 1300, 1300]


def test_d_add_new_matches_the_plain_restatement(cpu_hooks):
    g = _model()
    model = _snapshot(g)
    drawn = np.random.default_rng(1).integers(0, 30, size=50)
    assert g.add_new(5000, sampled=torch.from_numpy(drawn)) == 50 == ref.add_new_plain(model, drawn, 5000)
    _assert_equal(g, model)
    for name, attr in g._GROUP_OF.items():
        st = g.optimizer.state[getattr(g, attr)]
        assert not st['exp_avg'].numpy()[1000:].any() and not st['exp_avg_sq'].numpy()[np.unique(drawn)].any()
        assert getattr(g, attr).grad is None
    assert np.array_equal(g._positions.detach().numpy()[1000:], g._positions.detach().numpy()[drawn])


def test_d_the_draw_refuses_more_rows_than_multinomial_takes():
    with pytest.raises(RuntimeError, match='2\\^24'):
        gs._mcmc_draw(torch.empty(2 ** 24 + 1).as_strided((2 ** 24 + 1,), (0,)), 1)


# ---------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, name, **values):
    args = []
    for t, arg in protos[name][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, name)(*args)


def test_e_entry_points_are_exported_and_declared(lib):
    protos = _lib.parse_header()
    for name in SYMBOLS + ('nrc_gs_mcmc_regularise_ws_bytes',):
        assert name in protos and hasattr(lib, name), name
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 15


def test_e_bad_arguments_are_refused_before_any_device_call(lib):
    protos = _lib.parse_header()
    for name in SYMBOLS:
        assert _call(lib, protos, name, P=-1) == NRC_ERR_INVALID
        assert _call(lib, protos, name, P=1) == NRC_ERR_INVALID                # every required pointer is NULL
        assert _call(lib, protos, name, P=0) == NRC_OK                         # an empty model is a successful no-op
    assert _call(lib, protos, 'nrc_gs_mcmc_relocation', P=0, n_moments=12) == NRC_OK
    assert _call(lib, protos, 'nrc_gs_mcmc_relocation', P=0, n_moments=13) == NRC_ERR_INVALID
    assert _call(lib, protos, 'nrc_gs_mcmc_relocation', P=0, n_moments=-1) == NRC_ERR_INVALID
    assert _call(lib, protos, 'nrc_gs_mcmc_noise', P=0, row_offset=-1) == NRC_ERR_INVALID
    assert lib.nrc_gs_mcmc_regularise_ws_bytes(-1) == -1
    assert lib.nrc_gs_mcmc_regularise_ws_bytes(1) == 16 and lib.nrc_gs_mcmc_regularise_ws_bytes(257) == 32
    assert lib.nrc_gs_mcmc_regularise_ws_bytes(10 ** 9) == lib.nrc_gs_mcmc_regularise_ws_bytes(10 ** 8) == 2048 * 16       # the number of slabs is capped
    # one required pointer missing among otherwise non-null ones: still refused (the pointers are never dereferenced on this path)
    dummy = ctypes.c_void_p(64)
    full = dict(P=1, rotations=dummy, log_scales=dummy, opacity_logits=dummy, positions=dummy)
    for missing in ('rotations', 'log_scales', 'opacity_logits', 'positions'):
        assert _call(lib, protos, 'nrc_gs_mcmc_noise', **{k: v for k, v in full.items() if k != missing}) == NRC_ERR_INVALID
