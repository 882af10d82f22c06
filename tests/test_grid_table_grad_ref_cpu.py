"""CPU: the float64 table-gradient restatement of tests/grid_table_grad_ref.py is pinned (adjoint of input_grad_ref.grid_forward, agreement with the serial
f32 oracle inside the f32 budget), and the per-entry criterion is shown to bite: five seeded defects in an otherwise correct f32 result are all flagged,
three of which the tensor-maximum criterion the GPU tests used so far (rtol 2e-3, atol 2e-5 max|gradient|) lets through."""
import numpy as np
import pytest

import oracle
from tests import grid_table_grad_ref as R
from tests import input_grad_ref as I

CASES = [pytest.param(16, 2, 16, id='16x2-base16'), pytest.param(16, 2, 32, id='16x2-base32'), pytest.param(8, 4, 16, id='8x4')]
M = 6000


def _cfg(n_levels, n_features, base):
    return R.grid_cfg(n_levels, n_features, 14, base)


def _oracle_bw(x, d, cfg):
    kw = {k: cfg[k] for k in ('n_levels', 'log2_hashmap_size', 'base_resolution', 'per_level_scale')}
    return oracle.grid_encode_bw(x, d, R.n_entries(cfg), **kw)


_CACHE: dict = {}


def _case(n_levels, n_features, base, level_scale=None):
    key = (n_levels, n_features, base, None if level_scale is None else tuple(level_scale))
    if key not in _CACHE:
        cfg = _cfg(n_levels, n_features, base)
        x = I.positions(M, seed=n_levels + base)
        d = R.upstream(M, cfg, seed=3 * n_levels + base, level_scale=level_scale)
        G, A, n = R.table_grad(x, d, cfg)
        for a in (x, d, G, A, n):
            a.setflags(write=False)
        _CACHE[key] = (cfg, x, d, G, A, n)
    return _CACHE[key]


@pytest.mark.parametrize('n_levels,n_features,base', CASES)
def test_table_gradient_is_the_adjoint_of_the_forward_interpolation(n_levels, n_features, base):
    cfg, x, d, G, A, n = _case(n_levels, n_features, base)
    table = I.random_table(cfg, seed=5).astype(np.float64)
    lhs = float((I.grid_forward(x, table, cfg) * d.astype(np.float64)).sum())
    rhs = float((table * G).sum())
    print(f'adjoint identity {n_levels}x{n_features} base {base}: relative difference {abs(lhs - rhs) / abs(lhs):.2e}')
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert R.levels_have_addends(n, cfg)
    assert np.all((A > 0) == (n > 0)) and np.all(np.abs(G) <= A)


@pytest.mark.parametrize('n_levels,n_features,base', CASES)
def test_serial_f32_oracle_lies_within_the_f32_budget(n_levels, n_features, base):
    cfg, x, d, G, A, n = _case(n_levels, n_features, base)
    got = _oracle_bw(x, d, cfg)
    worst, over, moved = R.judge(got, G, n, R.budget_f32(A, n))
    print(f'oracle.grid_encode_bw {n_levels}x{n_features} base {base}: worst error / budget {worst:.3f}')
    assert over == 0 and moved == 0, (worst, over, moved)
    assert np.array_equal(got == 0, n == 0)


def _old_criterion_accepts(got, want):
    try:
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-5 * np.abs(want).max())
    except AssertionError:
        return False
    return True


def _flags(got, G, A, n):
    worst, over, moved = R.judge(got, G, n, R.budget_f32(A, n))
    return over > 0 or moved > 0


def _level_with_swapped_corners(x, d, cfg, level):
    """the level's table gradient with the weights of corners 0 and 1 exchanged (float64, level-local rows)"""
    _, offsets, scales, res = R._layout(cfg)
    F = cfg['n_features']
    gl = d[:, level * F:(level + 1) * F].astype(np.float64)
    rows = np.flatnonzero((gl != 0).any(1))
    cell, w1 = R._cells(x[rows], scales[level])
    w = np.stack([1.0 - w1, w1])
    size = int(offsets[level + 1] - offsets[level])
    out = np.zeros((size, F))
    for k in range(8):
        kw = {0: 1, 1: 0}.get(k, k)
        q = cell + np.array([k & 1, (k >> 1) & 1, k >> 2], np.uint32)
        wk = w[kw & 1, :, 0] * w[(kw >> 1) & 1, :, 1] * w[kw >> 2, :, 2]
        np.add.at(out, R._grid_index(q, int(res[level]), size), wk[:, None] * gl[rows])
    return out


def test_seeded_defects_are_flagged_and_three_of_them_pass_the_old_criterion():
    cfg, x, d, G, A, n = _case(16, 2, 16)
    _, offsets, _, _ = R._layout(cfg)
    good = _oracle_bw(x, d, cfg)
    assert not _flags(good, G, A, n) and _old_criterion_accepts(good, good)
    fine = slice(int(offsets[15]), int(offsets[16]))

    # 1: one sample's contribution to the finest level is missing (a live sample of median gradient there)
    mag = np.abs(d[:, 30:32]).max(1)
    live = np.flatnonzero(mag > 0)
    row = live[np.argsort(mag[live])[live.size // 2]]
    only = np.zeros_like(d[row:row + 1])
    only[:, 30:32] = d[row, 30:32]
    g1, _, n1 = R.table_grad(x[row:row + 1], only, cfg)
    assert n1.sum() > 0
    bad = (good.astype(np.float64) - g1).astype(np.float32)
    assert _flags(bad, G, A, n)
    assert _old_criterion_accepts(bad, good)

    # 2: the weights of two corners exchanged on one level
    bad = good.copy()
    bad[int(offsets[12]):int(offsets[13])] = _level_with_swapped_corners(x, d, cfg, 12).astype(np.float32)
    assert _flags(bad, G, A, n)

    # 4: one spurious addend where no sample lands
    e, f = np.argwhere(n[fine] == 0)[0]
    bad = good.copy()
    bad[int(offsets[15]) + e, f] = 1e-12
    assert _flags(bad, G, A, n)

    # 5: one level's values multiplied by 1 + 2^-10
    bad = good.copy()
    bad[fine] *= np.float32(1 + 2.0 ** -10)
    assert _flags(bad, G, A, n)
    assert _old_criterion_accepts(bad, good)

    # 3: a whole level lost whose gradients are 10^-6 of the other levels'
    scale = np.ones(16)
    scale[9] = 1e-6
    cfg, x, d, G, A, n = _case(16, 2, 16, level_scale=scale)
    good = _oracle_bw(x, d, cfg)
    assert not _flags(good, G, A, n)
    bad = good.copy()
    bad[int(offsets[9]):int(offsets[10])] = 0.0
    assert np.count_nonzero(good[int(offsets[9]):int(offsets[10])]) > 1000
    assert _flags(bad, G, A, n)
    assert _old_criterion_accepts(bad, good)
