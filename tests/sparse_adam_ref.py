"""Reference of the visibility-masked Adam step (nerficg_amd/csrc/adam_rows.hip, C ABI group 24), for the tests.

step_f32        numpy restatement of csrc/adam_math.h in float32 -- every operation rounded on its own, 1 - beta formed in float32, the operation order
                of the header -- applied to the rows a mask calls visible; the other rows are returned as they came.
published_f64   an independent float64 statement of the formula the published sparse kernels apply (3DGS `sparse_adam`, Taming-3DGS, gsplat
                `SelectiveAdam`): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p += -lr m / (sqrt(v) + eps), without bias correction.
compare         invisible rows bit for bit (view(int32)), visible rows within tolerance.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32

# tolerances of tests/test_gpu_adam_parity.py (same f32 operation order; sqrt and division correctly rounded)
TOL = {'p': dict(rtol=1e-6, atol=1e-7), 'm': dict(rtol=1e-6, atol=1e-12), 'v': dict(rtol=1e-6, atol=1e-20)}


def row_mask(mask, kind: int | None = None) -> np.ndarray:
    """Boolean (P,) row mask.  kind 0: bool / uint8, non-zero = visible; kind 1: int32 radii, > 0 = visible; None: by dtype."""
    mask = np.asarray(mask)
    if kind is None:
        kind = 1 if mask.dtype == np.int32 else 0
    if kind == 0:
        if mask.dtype not in (np.bool_, np.uint8):
            raise ValueError(f'kind 0 takes bool / uint8, got {mask.dtype}')
        return mask != 0
    if kind == 1:
        if mask.dtype != np.int32:
            raise ValueError(f'kind 1 takes int32, got {mask.dtype}')
        return mask > 0
    raise ValueError(f'unknown mask kind {kind}')


def step_f32(p, g, m, v, mask, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, adam_w_mode: bool = False,
             bias_correction: bool = True, kind: int | None = None):
    """(p, m, v) after one masked step number `step` (1-based; the GLOBAL count, as the optimizer keeps it).  p, g, m, v: (P, ...) float32; copies are returned."""
    p, m, v = (np.array(a, dtype=f32, copy=True) for a in (p, m, v))
    g = np.asarray(g, dtype=f32)
    vis = row_mask(mask, kind)
    if vis.shape != (p.shape[0],):
        raise ValueError(f'mask of shape {vis.shape} for {p.shape[0]} rows')
    b1, b2, lr_, eps_, wd = f32(betas[0]), f32(betas[1]), f32(lr), f32(eps), f32(weight_decay)
    # the bias corrections are formed on the host in double precision and handed over as float (FusedAdam: 1.0 - beta ** step, then c_float)
    bc1 = f32(1.0 - float(betas[0]) ** step) if bias_correction else f32(1.0)
    bc2 = f32(1.0 - float(betas[1]) ** step) if bias_correction else f32(1.0)
    one = f32(1.0)
    with np.errstate(all='ignore'):
        pr, gr, mr, vr = p[vis], g[vis].copy(), m[vis], v[vis]
        gr = gr * one                                            # g * inv_scale, inv_scale = 1
        if not adam_w_mode:
            gr = gr + wd * pr                                    # L2 mode
        mr = b1 * mr + (one - b1) * gr
        vr = b2 * vr + ((one - b2) * gr) * gr                    # C: (1 - beta2) * gr * gr associates to the left
        m_hat, v_hat = mr / bc1, vr / bc2
        update = m_hat / (np.sqrt(v_hat) + eps_)
        if adam_w_mode:
            update = update + wd * pr
        pr = pr - lr_ * update
    for a in (pr, mr, vr):
        assert a.dtype == f32
    p[vis], m[vis], v[vis] = pr, mr, vr
    return p, m, v


def published_f64(p, g, m, v, mask, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, kind: int | None = None):
    """The published sparse step in float64 on the float32 inputs (no bias correction, no weight decay); copies, invisible rows unchanged."""
    p, m, v = (np.array(a, dtype=np.float64, copy=True) for a in (p, m, v))
    g = np.asarray(g, dtype=np.float64)
    vis = row_mask(mask, kind)
    b1, b2 = float(f32(betas[0])), float(f32(betas[1]))          # the kernel receives the betas, lr and eps as floats
    lr, eps = float(f32(lr)), float(f32(eps))
    for r in np.nonzero(vis)[0]:
        m[r] = b1 * m[r] + (1.0 - b1) * g[r]
        v[r] = b2 * v[r] + (1.0 - b2) * g[r] * g[r]
        p[r] = p[r] + (-lr * m[r]) / (np.sqrt(v[r]) + eps)
    return p, m, v


def compare(before, after, expected, mask, kind: int | None = None, tol=TOL, what: str = '') -> None:
    """before / after / expected: (p, m, v) triples of (P, ...) float32 arrays.  Rows the mask calls invisible: `after` has the bits of `before`.
    Visible rows: `after` matches `expected` within tol.  AssertionError otherwise."""
    vis = row_mask(mask, kind)
    for name, b, a, e in zip(('p', 'm', 'v'), before, after, expected):
        b, a, e = (np.ascontiguousarray(x, dtype=f32) for x in (b, a, e))
        assert a.shape == b.shape == e.shape and a.shape[0] == vis.shape[0], f'{what} {name}: shapes {a.shape} {b.shape} {e.shape} mask {vis.shape}'
        same = a.view(np.int32) == b.view(np.int32)
        bad = ~same[~vis]
        assert not bad.any(), f'{what} {name}: {int(bad.sum())} elements of invisible rows changed their bits (first row {int(np.nonzero(~vis)[0][np.nonzero(bad.reshape(bad.shape[0], -1).any(1))[0][0]])})'
        np.testing.assert_allclose(a[vis], e[vis], err_msg=f'{what} {name}: visible rows', **tol[name])
