"""A float64 restatement and a per-entry error budget for the hash-grid TABLE gradient (nerficg_amd/csrc/ngp_net.hip: k_grid_bwd, k_grid_bwd_owned,
k_grid_bwd_owned_q, k_gb_split + k_gb_accumulate, k_grid_bwd_general).  Plain module: no test functions.  Used by tests/test_grid_table_grad_ref_cpu.py and
tests/test_gpu_grid_table_grad.py.  Layout, cells and corner indices are tests/input_grad_ref.py's (`_layout`, `_cells`, `_grid_index`), which that module's
tests pin against central differences of `grid_forward`.

The restatement
---------------
Per level: fx = fmaf(scale, x, 0.5) in f32 (reproduced exactly: positions are multiples of 2^-20 in [0, 1]), cell = floor(fx), w1 = fx - floor(fx) (exact
in f32), w0 = 1 - w1 in float64 (exact there).  Corner k = x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2) has the weight w_k = wx wy wz, and for every sample
whose F gradient components on the level are not all zero (the kernels skip the others) and every feature f
    G[entry_k, f] += w_k g_f          A[entry_k, f] += |w_k g_f|          n[entry_k, f] += (w_k g_f != 0)
all in float64.  n counts the NON-ZERO addends: a zero addend (a zero weight at an exact cell corner, or one zero component of a live sample) is one that
the kernels either skip or add as 0.0, which leaves the bits of a value that is not -0.0 as they were.  So "n == 0" is exactly "no sample moves this
value", and such a value must come back bit for bit as it went in.

The budget (u = 2^-24)
----------
Every operation below is counted as one rounding.  ngp_net.hip is built with the compiler's default contraction: a product that feeds an addition may
become one fma, which removes a rounding and never adds one.
gamma(c) = c u / (1 - c u), the usual bound of (1 + u)^c - 1; TINY = 2^-126, the smallest normal f32.

Every addend, on every path: 1 - w1 on three axes (3), two products for w_k (2), the product with g (1) = 6 roundings.  The f32 kernels form (wx wy) wz g
(grid_cell, ngp_net.h), the bucketed path ((wy wz) g) wx (k_gb_split's record, k_gb_accumulate's add_record): another association, the same count.

f32 paths.  The n addends of a value are summed in some order (the segmented scan over a run of equal cells in k_grid_bwd, LDS float atomics in the
ownership kernels, memory-side atomics), and the old value is part of that chain: every addend passes through at most n additions, each of which rounds
once.  So the addends carry at most n + 6 roundings:  gamma(n + 6) A.  The old value:
    ownership kernels   the slice is summed in LDS from 0 and added to the table ONCE: the old value meets one rounding                     u |old|
    global atomics      (k_grid_bwd, k_grid_bwd_general) the old value is the start of the chain and passes through every one of the
                        value's atomics, at most n of them                                                                                gamma(n) |old|
    err <= gamma(n + 6) A + {u | gamma(n)} |old| + 2 n TINY
The last term is the f32 format's lower end, not a rounding: a product w_k g or a partial sum below TINY is denormal, and float atomics may flush
denormals to zero; either way each of the at most 2 n operations that can produce one loses less than TINY.  (On the serial f32 oracle random data uses
0.4 of the budget.)

Bucketed path.  Every addend t (6 roundings) is multiplied by the power-of-two scale 2^s (exact) and rounded to the nearest integer: <= q/2 each, q = 2^-s,
    s = min(127, 62 - e_max - e_cnt),     max|g| < 2^e_max over the level's live rows (frexp),     2 M + 1 <= 2^e_cnt (frexp of float(2 M + 1)), M the row
capacity of the call -- the rule in the comment above k_gb_split; the clamp to 127 keeps the scale a finite f32 for levels whose largest gradient is
below 2^-(65 + e_cnt), which then resolve 2^-127.  The 64-bit integer sum is exact.  S = sum / 2^s goes through float64 (2^-53, counted with the next) to
f32: one rounding; old + S: one rounding, u |old + S| <= u |old| + u |S|.  So the addends carry 6 + 2 roundings:
    err <= gamma(8) A + n q/2 (1 + 2 u) + u |old| + 2 n TINY
(TINY as above: (wy wz) g and its product with wx can each be denormal before the scale is applied.)

No entry is excluded, and none is judged by anything but its own A, n and old value.
"""
from __future__ import annotations

import numpy as np

from tests.input_grad_ref import U, _cells, _grid_index, _layout, grid_cfg, grid_forward, n_entries  # noqa: F401  (re-exported for the tests)

TINY = 2.0 ** -126
OWN_OLD, ATOMIC_OLD = 'own', 'atomic'


def gamma(c):
    c = np.asarray(c, np.float64)
    return c * U / (1.0 - c * U)


def table_grad(x, d, cfg, live=None):
    """x (M, 3) f32 multiples of 2^-20; d (M, n_levels * F) f32, column level * F + f; live: only the first `live` rows count.
    Returns (G, A, n): (entries, F) float64, float64 and int64."""
    total, offsets, scales, res = _layout(cfg)
    F = cfg['n_features']
    m = x.shape[0] if live is None else int(live)
    x, d64 = x[:m], np.asarray(d[:m], np.float64)
    G, A, n = np.zeros((total, F)), np.zeros((total, F)), np.zeros((total, F), np.int64)
    for l in range(cfg['n_levels']):
        gl = d64[:, l * F:(l + 1) * F]
        rows = np.flatnonzero((gl != 0).any(1))
        if rows.size == 0:
            continue
        gl = gl[rows]
        cell, w1 = _cells(x[rows], scales[l])
        w = np.stack([1.0 - w1, w1])   # [0 / 1][rows][axis]
        size = int(offsets[l + 1] - offsets[l])
        for k in range(8):
            q = cell + np.array([k & 1, (k >> 1) & 1, k >> 2], np.uint32)
            idx = int(offsets[l]) + _grid_index(q, int(res[l]), size)
            t = (w[k & 1, :, 0] * w[(k >> 1) & 1, :, 1] * w[k >> 2, :, 2])[:, None] * gl
            np.add.at(G, idx, t)
            np.add.at(A, idx, np.abs(t))
            np.add.at(n, idx, (t != 0).astype(np.int64))
    return G, A, n


def budget_f32(A, n, old=None, old_path=OWN_OLD):
    """f32 paths; old_path: OWN_OLD (one read-modify-write per entry) or ATOMIC_OLD (the old value goes through every atomic)."""
    b = gamma(n + 6) * A + 2.0 * n * TINY
    if old is not None:
        b = b + (U if old_path == OWN_OLD else gamma(n)) * np.abs(np.asarray(old, np.float64))
    return np.where(n > 0, b, 0.0)


def fixed_point_lsb(d, cfg, level, capacity, live=None):
    """q of the bucketed path for one level: d (M, n_levels * F) f32 as in table_grad, capacity the M passed to the call."""
    F = cfg['n_features']
    m = d.shape[0] if live is None else int(live)
    gl = np.abs(d[:m, level * F:(level + 1) * F])
    mx = np.float32(gl.max()) if gl.size else np.float32(0.0)
    e_max = int(np.frexp(mx if mx > 0 else np.float32(1.0))[1])
    e_cnt = int(np.frexp(np.float32(2 * capacity + 1))[1])
    return 2.0 ** -min(127, 62 - e_max - e_cnt)


def budget_bucketed(A, n, q, old=None):
    """q: (entries, 1) or scalar fixed-point LSB of each entry's level."""
    b = gamma(8) * A + n * (q / 2.0) * (1.0 + 2.0 * U) + 2.0 * n * TINY
    if old is not None:
        b = b + U * np.abs(np.asarray(old, np.float64))
    return np.where(n > 0, b, 0.0)


def judge(got, G, n, budget, old=None):
    """(worst err / budget over the entries with addends, number of entries over budget, number of n == 0 entries whose bits changed).
    got, old: (entries, F) f32."""
    got = np.asarray(got, np.float32)
    want = G if old is None else G + np.asarray(old, np.float64)
    err = np.abs(got.astype(np.float64) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    touched = n > 0
    before = np.zeros_like(got) if old is None else np.asarray(old, np.float32)
    moved = int(np.count_nonzero((got.view(np.uint32) != before.view(np.uint32)) & ~touched))
    over = int(np.count_nonzero(err[touched] > budget[touched]))
    worst = float((err[touched] / budget[touched]).max()) if touched.any() else 0.0
    return worst, over, moved


def levels_have_addends(n, cfg):
    _, offsets, _, _ = _layout(cfg)
    return all(bool((n[offsets[l]:offsets[l + 1]] > 0).any()) for l in range(cfg['n_levels']))


def level_of_entry(cfg):
    """(entries,) int: the level every table entry belongs to"""
    total, offsets, _, _ = _layout(cfg)
    return np.repeat(np.arange(cfg['n_levels']), np.diff(offsets))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def quantise(x):
    """positions -> f32 multiples of 2^-20 in [0, 1]"""
    return (np.round(np.clip(np.asarray(x, np.float64), 0.0, 1.0) * 2.0 ** 20) / 2.0 ** 20).astype(np.float32)


def upstream(m, cfg, seed, level_scale=None, zero_rows=0.25):
    """(m, n_levels * F) f32: normal values times 10^-6 .. 1 per (sample, level), times a per-level factor (default 10^(-l/4): the fine levels' gradients
    are orders of magnitude below the coarse levels'); a share `zero_rows` of the rows, never the first, is all zero."""
    rng = np.random.default_rng(seed)
    L, F = cfg['n_levels'], cfg['n_features']
    if level_scale is None:
        level_scale = 10.0 ** (-np.arange(L) / 4.0)
    g = rng.normal(size=(m, L, F)) * 10.0 ** rng.uniform(-6, 0, size=(m, L, 1)) * np.asarray(level_scale, np.float64)[None, :, None]
    dead = rng.random(m) < zero_rows
    dead[0] = False   # (a one-row batch is a live one)
    g[dead] = 0.0
    return g.reshape(m, L * F).astype(np.float32)
