"""CPU: the comparison of tests/ssim_cases.py has teeth.  A float64 numpy SSIM is pinned against oracle/ssim_oracle.c, wrong variants of it
must be rejected by `assert_within_budget`, and an f32 emulation of the kernel's arithmetic (same tap order, np.float32 accumulators, no
FMA -- ssim.hip is built with the default contraction, so an approximation) must pass: the budget is neither too loose for a wrong kernel
nor too tight for a correct f32 one."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from tests import ssim_cases as sc

NAMES = ('map', 'dm_dmu1', 'dm_dsigma1_sq', 'dm_dsigma12', 'grad')


@functools.lru_cache(maxsize=None)
def _case(name, shape=None):
    """Inputs, the oracle's five outputs and their budgets; computed once and shared (nothing writes into them)."""
    shape = shape or sc.case_shape(name)
    seed = sc.case_seed(name)
    a, b = sc.BUILDERS[name](shape, seed)
    w = sc.upstream(shape, seed)
    m, d1, d2, d3 = oracle.ssim_forward(a, b)
    ref = dict(zip(NAMES, (m, d1, d2, d3, oracle.ssim_backward(a, b, w, d1, d2, d3))))
    for v in (a, b, w, *ref.values()):
        v.setflags(write=False)
    return a, b, w, ref, sc.ssim_budget(a, b, w)


def _model(a, b, w, dtype=np.float64, shift=False, plane_roll=False, **kw):
    """The numpy model's five outputs.  `shift`: both images read one pixel to the right (a halo off-by-one); `plane_roll`: every plane read
    from its neighbour's offset."""
    if shift:
        a, b = (np.concatenate([v[..., 1:], np.zeros_like(v[..., :1])], axis=-1) for v in (a, b))
    if plane_roll:
        a, b = (np.roll(v.reshape((-1,) + v.shape[-2:]), -1, axis=0).reshape(v.shape) for v in (a, b))
    g = kw.pop('g', sc.KERNEL_WINDOW if dtype == np.float32 else None)
    f = sc.model_forward(a, b, g=g, dtype=dtype, **kw)
    return dict(zip(NAMES, (*f, sc.model_backward(a, b, w, *f[1:], g=g, dtype=dtype))))


def _last_tap_dropped():
    g = sc.gauss_window().copy()
    g[10] = 0.0
    return g


MUTANTS = {
    'C2 x 1.05': dict(c2=1.05 * sc.C2),
    'C1 and C2 swapped': dict(c1=sc.C2, c2=sc.C1),
    'sigma 1.55': dict(g=sc.gauss_window(1.55)),
    'shifted one pixel in x': dict(shift=True),
    'variance as E[x^2] - mu1 mu2': dict(variance_bug=True),
    "plane from its neighbour's offset": dict(plane_roll=True),
    'last tap dropped': dict(g=_last_tap_dropped()),
}
# which builders must reject which mutant (the whole matrix is in test_mutant_matrix's output: run with -s)
EXPECTED_REJECTIONS = {
    'C2 x 1.05': ('noise', 'grey_whisper', 'flat_white'),
    'C1 and C2 swapped': ('noise', 'flat_black', 'grey_whisper'),
    'sigma 1.55': ('noise', 'silhouette', 'planes_differ'),
    'shifted one pixel in x': ('noise', 'silhouette', 'planes_differ'),
    'variance as E[x^2] - mu1 mu2': ('noise', 'out_of_range', 'planes_differ'),
    "plane from its neighbour's offset": ('noise', 'planes_differ', 'silhouette'),
    'last tap dropped': ('noise', 'flat_white', 'grey_whisper'),
}


def _rejected(name, mutant):
    a, b, w, ref, bud = _case(name)
    got = _model(a, b, w, **MUTANTS[mutant])
    failed = []
    for k in NAMES:
        try:
            sc.assert_within_budget(got[k], ref[k], bud[k], f'{mutant} / {name} / {k}')
        except AssertionError:
            failed.append(k)
    return failed


def test_window_constants_of_the_kernel_are_the_f32_of_the_oracles_window():
    """The budget takes the window constants' error from ssim_cases.KERNEL_WINDOW: that must be ssim.hip's SSIM_G, and stay within 1.5 u of
    the oracle's double window."""
    text = (Path(__file__).resolve().parents[1] / 'nerficg_amd' / 'csrc' / 'ssim.hip').read_text()
    body = re.search(r'SSIM_G\[11\]\s*=\s*\{([^}]*)\}', text).group(1)
    consts = np.array([float(v.rstrip('f')) for v in body.replace('\n', ' ').split(',')]).astype(np.float32)
    assert np.array_equal(consts, sc.KERNEL_WINDOW)
    assert sc.WINDOW_ERROR_U.max() < 1.5


@pytest.mark.parametrize('name', sorted(sc.BUILDERS))
def test_builders_are_seeded_f32_pairs(name):
    shape = sc.case_shape(name)
    a, b = sc.BUILDERS[name](shape, 5)
    a2, b2 = sc.BUILDERS[name](shape, 5)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == shape
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    if name == 'planes_differ':   # no two planes interchangeable: means apart by more than the pattern's noise, contents different
        p = a.reshape((-1,) + shape[-2:]).astype(np.float64)
        means = np.sort(p.mean(axis=(1, 2)))
        assert np.diff(means).min() > 0.1
    if name in ('flat_white', 'flat_black'):
        level = 1.0 if name == 'flat_white' else 0.0
        assert (b == level).all() and (a == level).mean() > 0.5 and (a != level).any()
    if name == 'identical':
        assert np.array_equal(a, b)
    if name == 'out_of_range':
        assert a.min() < -0.2 and a.max() > 1.4


@pytest.mark.parametrize('name', sorted(sc.BUILDERS))
def test_numpy_model_agrees_with_the_oracle(name):
    """float64 model == the oracle before its f32 store: |model - oracle| <= half an f32 ulp of the model + the double rounding of two
    different summation orders.  The latter is the f32 budget scaled by 2^-53 / 2^-24 (the same conditioning, the unit roundoff of double):
    ~1e-13 on noise, up to ~1e-8 for derivative maps of size 1e3 on the flat builders, where 1 / B amplifies every rounding a thousandfold."""
    a, b, w, ref, bud = _case(name)
    got = _model(a, b, w)
    # the oracle's backward pass reads its own f32 maps: feed the model the same ones
    got['grad'] = sc.model_backward(a, b, w, *(ref[k].astype(np.float64) for k in NAMES[1:4]))
    for k in NAMES:
        r = ref[k].astype(np.float64)
        tol = sc.U * np.abs(got[k]) * (1 + 1e-9) + 2.0 ** -29 * bud[k]
        worst = np.max(np.abs(got[k] - r) - tol)
        assert worst <= 0, (k, worst)


@pytest.mark.parametrize('name', sorted(sc.BUILDERS))
def test_f32_emulation_passes_the_budget(name):
    a, b, w, ref, bud = _case(name)
    got = _model(a, b, w, dtype=np.float32)
    ratios = {k: sc.assert_within_budget(got[k], ref[k], bud[k], f'f32 emulation / {name} / {k}') for k in NAMES}
    print(f'f32 emulation err/budget {name}: ' + ' '.join(f'{k}={v:.3f}' for k, v in ratios.items()))
    if name == 'noise':   # common ground with test_gpu_ssim_parity.py: a correct f32 kernel also meets the old absolute tolerances
        assert np.abs(got['map'] - ref['map']).max() < 2e-6
        assert np.abs(got['grad'] - ref['grad']).max() < 2e-5 * np.abs(ref['grad']).max()


@pytest.mark.parametrize('shape', [(1, 2, 1, 1), (1, 2, 1, 65), (1, 2, 65, 1), (1, 2, 11, 43), (1, 2, 33, 32)])
@pytest.mark.parametrize('name', ['noise', 'flat_white'])
def test_f32_emulation_passes_the_budget_at_tile_edge_shapes(name, shape):
    a, b, w, ref, bud = _case(name, shape)
    got = _model(a, b, w, dtype=np.float32)
    for k in NAMES:
        sc.assert_within_budget(got[k], ref[k], bud[k], f'f32 emulation / {name} {shape} / {k}')


@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_every_mutant_is_rejected(mutant):
    for name in EXPECTED_REJECTIONS[mutant]:
        assert _rejected(name, mutant), f'{mutant} passes the budget on {name}'


def test_mutant_matrix():
    """The whole matrix, printed for the record (-s); asserts only that no mutant survives every builder."""
    lines = []
    for mutant in MUTANTS:
        row = {name: _rejected(name, mutant) for name in sc.BUILDERS}
        assert any(row.values()), f'{mutant} passes everywhere'
        lines.append(f'{mutant:36s} ' + ' '.join(f'{name}:{len(f)}' for name, f in row.items()))
    print('\nmutant x builder: outputs rejected (of 5)\n' + '\n'.join(lines))


def test_assert_within_budget_checks_every_element_and_reports_the_worst():
    ref = np.zeros((2, 3))
    bud = np.full((2, 3), 1e-3)
    got = ref.copy()
    got[0, 1] = 5e-4
    assert sc.assert_within_budget(got, ref, bud, 'x') == pytest.approx(0.5)
    got[1, 2] = 2e-3
    with pytest.raises(AssertionError, match=r'x: element \(1, 2\) got 0\.002 ref 0\.0 .*budget 1\.000e-03'):
        sc.assert_within_budget(got, ref, bud, 'x')
    for bad in (np.nan, np.inf):
        got = ref.copy()
        got[0, 0] = bad
        with pytest.raises(AssertionError, match=r'element \(0, 0\)'):
            sc.assert_within_budget(got, ref, bud, 'x')
    bud0 = bud.copy()
    bud0[1, 0] = 0.0                       # a zero budget admits only an exact match
    assert sc.assert_within_budget(ref, ref, bud0, 'x') == 0.0
    got = ref.copy()
    got[1, 0] = 1e-30
    with pytest.raises(AssertionError, match=r'element \(1, 0\)'):
        sc.assert_within_budget(got, ref, bud0, 'x')
    with pytest.raises(AssertionError):
        sc.assert_within_budget(ref[:1], ref, bud, 'x')
