"""Inputs, a float64 restatement and a per-element f32 error budget for the input-gradient kernels (nerficg_amd/csrc/ngp_input_grad.hip:
nrc_grid_backward_input, nrc_sh_identity_backward_input).  Plain module: no test functions.  Used by tests/test_input_grad_ref_cpu.py and
tests/test_gpu_input_grad.py.

The restatement
---------------
Grid.  Level scales, resolutions and offsets come from oracle.grid_layout; the corner index is oracle/tcnn_oracle.c's grid_index (dense x + y res +
z res^2 while the running stride fits the level, the spatial hash otherwise, modulo the level size).  The cell and the fractions follow the f32 chain of
grid_cell (ngp_net.h): fx = fmaf(scale, x, 0.5) in f32, cell = floor(fx), fraction = fx - floor(fx) (exact in f32).  Test positions are multiples of 2^-20
in [0, 1]: scale (24 bits) times x (21 bits) plus 0.5 is then exact in float64, and ONE rounding of it to f32 is the fmaf.  Everything behind that is float64:
    s_k = sum_f g_f v_k[f]                         (corner k = x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2); v fp16 table values, g the upstream gradient)
    d/dx = scale sum over the four (y, z) corner pairs of  wy wz (s_k1 - s_k0),     likewise y and z,        summed over the levels
-- the piecewise derivative of the cell the forward pass used; the forward's final fp16 rounding of the feature is ignored, as tiny-cuda-nn does.  Both sides
take the same floor, so no position is excluded: exact 0, exact 1 and exact cell corners are ordinary inputs.
`grid_forward(..., shift=delta)` evaluates the same interpolant at the position displaced by a float64 `delta` BEHIND the f32 chain (fx = f32(scale x + 0.5) +
scale delta, so that the other axes' fractions stay the forward pass's own): the function of delta whose central differences at 0
tests/test_input_grad_ref_cpu.py compares the derivative with.

SH.  The 16 polynomials of sh4_eval / oracle/tcnn_oracle.c:198-215 in torch float64 at d = 2 d01 - 1, differentiated by torch autograd.

The budget
----------
err <= c u sum|addends|, u = 2^-24, where the sum of the absolute values of every addend is accumulated alongside the value.  The translation unit is built
with -ffp-contract=off: every operation below rounds once, nothing is fused that is not written as fmaf.

Grid, per output element; A_k = sum_f |g_f v_k[f]|, addend of a corner pair = scale w (A_k1 + A_k0), w the product of the two other axes' weights:
    s_k    gl0 * v0, then F - 1 fmaf: F roundings, each <= u A_k                                         -> F u A_k
    diff   s_k1 - s_k0: the two operands' errors + one rounding u |diff| <= u (A_k1 + A_k0)              -> (F + 1) u (A_k1 + A_k0)
    w      1 - w1 (one rounding, each axis), the product (one): relative 3 u; w * diff (one): 4 u         -> (F + 5) u w (A_k1 + A_k0)
    sum    four addends as (t0 + t1) + (t2 + t3): counted as 3 additions over sum|t|                     -> + 3 u
    scale  scale * sum: one rounding                                                                     -> + 1 u
    levels a wave adds at most 4 levels (<= 3 roundings: the first lands on 0), the 4 waves' partials 3 more additions, each <= u sum|addends|  -> + 6 u
  c = F + 15, and one more for the second-order terms of (1 + u)^c:      GRID_C(F) = F + 16.     The fp16 table values and the f32 gradient are exact inputs.

SH, per direction component; J_abs = the derivative polynomial with every monomial taken absolute, addend = 2 |g_c| J_abs_c:
    J      constants in f32 (<= 2 roundings: c5 and 6 c5), the monomial (x y, z^2: 1), a scaled difference like 3 y^2 - 3 x^2 (<= 3 along a path), the product
           with the constant (1): <= 5 relative to J_abs;  g * J: one more                                -> 6 u
    sum    nine terms: 8 additions, each <= u sum|addends|                                               -> + 8 u          (d = 2 d01 - 1 and the final * 2 are exact)
  c = 14, and one more for second order:                                 SH_C = 15.
Columns 3..18 of the SH entry point are copies of d_in[16:32]: exact.
"""
from __future__ import annotations

import numpy as np

import oracle

U = 2.0 ** -24
SH_C = 15
PLS = float(np.exp(np.log(2048 * 1.0 / 16) / 15))   # the shipped grid's growth (Model.py:68 with SCALE 0.5)


def GRID_C(n_features: int) -> int:
    return n_features + 16


def grid_cfg(n_levels, n_features, log2_hashmap_size=19, base_resolution=16, per_level_scale=PLS) -> dict:
    return dict(n_levels=n_levels, n_features=n_features, log2_hashmap_size=log2_hashmap_size, base_resolution=base_resolution, per_level_scale=per_level_scale)


def _layout(cfg):
    total, offsets, scales, res = oracle.grid_layout(cfg['n_levels'], cfg['log2_hashmap_size'], cfg['base_resolution'], cfg['per_level_scale'])
    return total, offsets.astype(np.int64), scales.astype(np.float32), res.astype(np.int64)


def n_entries(cfg) -> int:
    return _layout(cfg)[0]


def _grid_index(q, res: int, size: int):
    """oracle/tcnn_oracle.c grid_index on (M, 3) uint32 corner coordinates, uint32 arithmetic (the running stride stays below 2^32 for every level size <= 2^30
    this module is used with: res^2 <= size there)."""
    stride, index = 1, np.zeros(q.shape[0], np.uint32)
    for d in range(3):
        if stride <= size:
            index = index + q[:, d] * np.uint32(stride)
            stride *= res
    assert stride < 2 ** 32
    if size < stride:
        index = q[:, 0] ^ (q[:, 1] * np.uint32(2654435761)) ^ (q[:, 2] * np.uint32(805459861))
    return (index % np.uint32(size)).astype(np.int64)


def _cells(x, scale: np.float32, shift=None):
    """(cell (M,3) uint32, fraction (M,3) f64) of positions x at a level; `shift` (3,) float64 displaces the position behind the f32 chain."""
    assert x.dtype == np.float32 and np.all(x.astype(np.float64) * 2.0 ** 20 == np.round(x.astype(np.float64) * 2.0 ** 20)), 'positions must be multiples of 2^-20'
    fx = (np.float64(scale) * x.astype(np.float64) + 0.5).astype(np.float32)     # exact in f64, one rounding: the fmaf
    if shift is None:
        fl = np.floor(fx)
        return fl.astype(np.int32).astype(np.uint32), (fx - fl).astype(np.float64)  # (fx - fl is exact in f32)
    fx = fx.astype(np.float64) + np.float64(scale) * np.asarray(shift, np.float64)
    fl = np.floor(fx)
    return fl.astype(np.int64).astype(np.uint32), fx - fl


def _corner_values(cell, table64, level_offset: int, res: int, size: int):
    """(8, M, F) float64 table values of the cell's corners in Corner8 order."""
    out = []
    for k in range(8):
        q = cell + np.array([k & 1, (k >> 1) & 1, k >> 2], np.uint32)
        out.append(table64[level_offset + _grid_index(q, res, size)])
    return np.stack(out)


def grid_forward(x, table, cfg, shift=None):
    """(M, n_levels * F) float64 features (no fp16 rounding), column level * F + c.  table: (entries, F) fp16-representable."""
    _, offsets, scales, res = _layout(cfg)
    t64 = np.asarray(table, np.float64)
    F = t64.shape[1]
    out = np.zeros((x.shape[0], cfg['n_levels'] * F))
    for l in range(cfg['n_levels']):
        cell, w1 = _cells(x, scales[l], shift)
        v = _corner_values(cell, t64, int(offsets[l]), int(res[l]), int(offsets[l + 1] - offsets[l]))
        w = np.stack([1.0 - w1, w1])   # [0 / 1][M][axis]
        for k in range(8):
            wk = w[k & 1, :, 0] * w[(k >> 1) & 1, :, 1] * w[k >> 2, :, 2]
            out[:, l * F:(l + 1) * F] += wk[:, None] * v[k]
    return out


def grid_input_grad(x, d_features, table, cfg):
    """x (M,3) f32 multiples of 2^-20; d_features (M, n_levels * F) f32, column level * F + c; table (entries, F) fp16-representable.
    Returns (gradient (M,3) float64, sum of |addends| (M,3) float64); the budget of an element is GRID_C(F) * U * that sum."""
    _, offsets, scales, res = _layout(cfg)
    t64 = np.asarray(table, np.float64)
    F = t64.shape[1]
    g64 = np.asarray(d_features, np.float64)
    grad, mag = np.zeros((x.shape[0], 3)), np.zeros((x.shape[0], 3))
    for l in range(cfg['n_levels']):
        cell, w1 = _cells(x, scales[l])
        v = _corner_values(cell, t64, int(offsets[l]), int(res[l]), int(offsets[l + 1] - offsets[l]))
        gl = g64[:, l * F:(l + 1) * F]
        s = (gl[None] * v).sum(-1)            # (8, M)
        a = np.abs(gl[None] * v).sum(-1)
        w = np.stack([1.0 - w1, w1])
        sc = np.float64(scales[l])
        for axis in range(3):
            b, c = [d for d in range(3) if d != axis]
            for ib in range(2):
                for ic in range(2):
                    k0 = (ib << b) | (ic << c)
                    k1 = k0 | (1 << axis)
                    wk = w[ib, :, b] * w[ic, :, c]
                    grad[:, axis] += sc * wk * (s[k1] - s[k0])
                    mag[:, axis] += sc * wk * (a[k1] + a[k0])
    return grad, mag


# ---- SH degree 4 ---------------------------------------------------------------------------------------------------------------------------------------
C1, C2, C3, C4, C5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.54627421529603959, 0.59004358992664352
C6, C7, C8, C9 = 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769


def sh4_torch(d01):
    """(M, 16) torch float64 coefficients at d = 2 d01 - 1 (d01 a float64 tensor): oracle/tcnn_oracle.c:198-215."""
    import torch
    d = 2.0 * d01 - 1.0
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return torch.stack([torch.full_like(x, 0.28209479177387814), -C1 * y, C1 * z, -C1 * x, C2 * xy, -C2 * yz, C3 * z2 - 0.31539156525251999, -C2 * xz,
                        C4 * x2 - C4 * y2, C5 * y * (-3.0 * x2 + y2), C6 * xy * z, C7 * y * (1.0 - 5.0 * z2), C8 * z * (5.0 * z2 - 3.0), C7 * x * (1.0 - 5.0 * z2),
                        C9 * z * (x2 - y2), C5 * x * (-x2 + 3.0 * y2)], dim=1)


def sh_input_grad(d01_half, g16):
    """d01_half (M,3): the fp16 input values (any float dtype); g16 (M,16): upstream gradient of the 16 coefficients.  Returns (gradient w.r.t. d01 (M,3)
    float64 by torch autograd, sum of |addends| (M,3) float64); the budget of an element is SH_C * U * that sum."""
    import torch
    d01 = torch.tensor(np.asarray(d01_half, np.float64), dtype=torch.float64, requires_grad=True)
    (sh4_torch(d01) * torch.tensor(np.asarray(g16, np.float64))).sum().backward()
    d = 2.0 * np.asarray(d01_half, np.float64) - 1.0
    x, y, z = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    g = np.abs(np.asarray(g16, np.float64))
    q5, q3 = C7 * (1.0 + 5.0 * z * z), C5 * (3.0 * x * x + 3.0 * y * y)
    mx = g[:, 3] * C1 + g[:, 4] * C2 * y + g[:, 7] * C2 * z + g[:, 8] * 2 * C4 * x + g[:, 9] * 6 * C5 * x * y + g[:, 10] * C6 * y * z + g[:, 13] * q5 + \
        g[:, 14] * 2 * C9 * x * z + g[:, 15] * q3
    my = g[:, 1] * C1 + g[:, 4] * C2 * x + g[:, 5] * C2 * z + g[:, 8] * 2 * C4 * y + g[:, 9] * q3 + g[:, 10] * C6 * x * z + g[:, 11] * q5 + \
        g[:, 14] * 2 * C9 * y * z + g[:, 15] * 6 * C5 * x * y
    mz = g[:, 2] * C1 + g[:, 5] * C2 * y + g[:, 6] * 2 * C3 * z + g[:, 7] * C2 * x + g[:, 10] * C6 * x * y + g[:, 11] * 10 * C7 * y * z + \
        g[:, 12] * C8 * (15.0 * z * z + 3.0) + g[:, 13] * 10 * C7 * x * z + g[:, 14] * C9 * (x * x + y * y)
    return d01.grad.numpy(), 2.0 * np.stack([mx, my, mz], axis=1)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
SPECIAL_POSITIONS = np.array([[0.0, 1.0, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.5, 0.0, 1.0]], np.float32)
# (0.5 is an exact cell corner of level 0 for base_resolution 16: 15 * 0.5 + 0.5 = 8; 0 and 1 are the faces of the box)


def positions(m: int, seed: int):
    """(m, 3) f32 multiples of 2^-20 in [0, 1]; the first rows are SPECIAL_POSITIONS (exact 0, exact 1, exact cell corners)."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 2 ** 20 + 1, size=(m, 3)).astype(np.float64) / 2.0 ** 20).astype(np.float32)
    k = min(m, len(SPECIAL_POSITIONS))
    x[:k] = SPECIAL_POSITIONS[:k]
    return x


def random_table(cfg, seed: int):
    """(entries, F) float32 holding random fp16 values in [-1, 1]."""
    rng = np.random.default_rng(seed)
    return (rng.random((n_entries(cfg), cfg['n_features']), dtype=np.float32) * 2 - 1).astype(np.float16).astype(np.float32)


def upstream(m: int, width: int, seed: int):
    """(m, width) f32 normal values spread over six decades; every row i with i % 4 == 1 is all zero (interleaved with live rows)."""
    rng = np.random.default_rng(seed)
    g = (rng.normal(size=(m, width)) * 10.0 ** rng.integers(-5, 1, size=(m, 1))).astype(np.float32)
    g[1::4] = 0.0
    return g
