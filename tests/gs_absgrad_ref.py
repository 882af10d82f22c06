"""A float64 reference and the per-element budget for the absolute screen-space gradients of the 3DGS rasterizer (absgrad: k_render_bw<., true> of
nerficg_amd/csrc/gs_raster.hip, C ABI group 23).  Plain module: no test functions.  Used by tests/test_gs_absgrad_ref_cpu.py and tests/test_gpu_gs_absgrad.py.

Definition.  With the addends exactly as gs_grad_ref.BlendRef.sums states them (add[4], add[5]), for Gaussian i
    abs_x[i] = sum over tiles and the pixels that blended i of | -w (dx A + dy B) W/2 |        abs_y[i] = sum ... of | -w (dy C + dx B) H/2 |
w = o G dL/dalpha of the whole call (colour, and with the maps the depth and alpha channels).  The absolute value is taken PER PIXEL, before any row, block,
tile or band sum.  `addends` repeats the walk of BlendRef.sums (same forward decisions, same T, same running colour, same dL/dalpha) and yields the two
addends per (tile, entry) over the tile's pixels; `want_abs` sums their magnitudes.  tests/test_gs_absgrad_ref_cpu.py holds the walk against an independent
torch autograd statement and against S of BlendRef.sums (the signed sum of the same addends).

Budget.  The budget of abs_x, abs_y is blend_budget(...)[:, 4:6] of gs_grad_ref UNCHANGED -- the budget of the signed sums mean_x, mean_y:
    B_q = R_q + gamma(tiles + 2) A_q + fixed_q + tiny_q            (q = 4, 5; the docstring of gs_grad_ref.py derives every term)
It bounds the new sums term by term:
  R_q    For one addend, | |a32| - |a64| | <= |a32 - a64| (reverse triangle inequality), and fabsf is exact: the float32 error of |addend| is at most that of
         the addend, rel(pixel, entry) |addend| with the addend's magnitude as in A.  The row reduction of the |.| values is four DPP adds (mirror, half
         mirror, two quad permutations), the four that C1 counts for the longest column.  R_q is a sum of per-addend bounds: it does not rely on any
         cancellation, so it holds for the sum of magnitudes as for the signed sum.
  gamma(tiles + 2) A_q    The flush is the same conversion to float32, the same constant (W/2, H/2 times 2^(gexp - BW_S_MEAN), without the sign) and the same
         one float atomic per (tile, Gaussian): tiles + 2 roundings of partial sums, each at most sum |addend| <= A_q in magnitude.
  fixed_q   `deposit` truncates the scaled row sum: less than one step of the mean class per depositing (tile, block) pair -- the same pairs (a block deposits
         for an entry iff one of its pixels blends it), the same step 2^(gexp_t - BW_S_MEAN) W/2 | H/2.
  tiny_q    the float32 format's lower end: the same products.
No new constant is introduced.  A_q >= want_abs >= |S_q| (A_q replaces dx A + dy B by |dx A| + |dy B| and c - n by |c| + |n|), so A == 0 means exactly zero:
culled Gaussians and Gaussians no pixel blended.  The fixed-point class: BW_S_MEAN's bound was derived from the magnitudes of the addends (terms that may all
have one sign), so the sum of magnitudes does not exceed it either."""
from __future__ import annotations

import numpy as np

from tests import gs_grad_ref as R


def addends(blend, g, g_d=None, g_a=None):
    """Yields (tile, i, active (N,) bool, add (2, N) float64): entry i of `tile`, the pixels that blended it and the addends of mean2D x, y over the tile's N
    pixels (zero where not active) -- the walk of BlendRef.sums.  g (3, H, W) float32, already masked; with the maps g_d, g_a (H, W)."""
    f = np.float64
    g = np.asarray(g)
    assert g.dtype == np.float32 and g.shape == (3, blend.H, blend.W)
    assert not g[:, blend.ambiguous].any(), 'mask the gradients first (mask_ambiguous)'
    if blend.aux:
        g_d, g_a = np.asarray(g_d), np.asarray(g_a)
        assert g_d.dtype == g_a.dtype == np.float32 and not g_d[blend.ambiguous].any() and not g_a[blend.ambiguous].any()
    hW, hH = 0.5 * blend.W, 0.5 * blend.H
    bg = blend.bg
    for tl in blend.tiles:
        gmax, _ = blend.tile_gexp(tl, g, g_d, g_a)
        if not gmax > 0:
            continue
        gv = [g[c, tl.py, tl.px].astype(f) for c in range(3)]
        if blend.aux:
            gv += [g_d[tl.py, tl.px].astype(f), g_a[tl.py, tl.px].astype(f)]
        gv = np.stack(gv)
        Tf = blend.T_final[tl.py, tl.px]
        bgdot = (bg[:, None] * gv[:3]).sum(0)
        T = Tf.copy()
        n = np.zeros_like(gv)
        for k in range(tl.ids.size - 1, -1, -1):
            a = tl.active[k]
            if not a.any():
                continue
            al, G, dx, dy = tl.al[k], np.where(a, tl.G[k], 0.0), tl.dx[k], tl.dy[k]
            cA, cB, cC, o = tl.co[k]
            r = 1.0 / (1.0 - al)
            T = T * r
            e = tl.c[k][:, None] - n
            dLda = (e * gv).sum(0) * T - Tf * bgdot * r
            wg = o * G * dLda
            yield tl, int(tl.ids[k]), a, np.stack([-wg * (dx * cA + dy * cB) * hW, -wg * (dy * cC + dx * cB) * hH])
            n = n + al * e


def want_abs(blend, g, g_d=None, g_a=None):
    """(P, 2) float64: abs_x, abs_y of the definition."""
    out = np.zeros((blend.P, 2), np.float64)
    for _, i, _, add in addends(blend, g, g_d, g_a):
        out[i] += np.abs(add).sum(1)
    return out


def budget(B):
    """The budget of (abs_x, abs_y) from blend_budget's B (P, NQ): its columns of mean_x, mean_y, unchanged."""
    return B[:, 4:6]


def magnitude(ref):
    """A of (abs_x, abs_y) from BlendRef.sums' dict: the magnitude columns of mean_x, mean_y (zero exactly where the result must be exactly zero)."""
    return ref['A'][:, 4:6]


def judge(got, want, B, A):
    """gs_grad_ref.judge on the (P, 2) pair: (worst err / budget, elements over budget, A == 0 elements that are not exactly zero)."""
    return R.judge(np.asarray(got, np.float64)[:, :2], want, B, A)
