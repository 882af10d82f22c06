"""A float64 restatement and per-element error budgets for the per-Gaussian contribution statistics of the 3DGS rasterizer (nerficg_amd/csrc/gs_contrib.hip:
k_gs_contributions).  Plain module: no test functions.  Used by tests/test_gs_contrib_ref_cpu.py and tests/test_gpu_gs_contributions.py.

The statement
-------------
The blended set of a pixel, alpha, T and w = alpha T are BlendRef's (tests/gs_grad_ref.py): the list entries in front of n_contrib with power <= 0 and
alpha >= 1/255, in float64 (tl.al, tl.active, tl.ids of its tiles).  m is an (H, W) float32 map, promoted; a pixel PARTICIPATES iff m(p) != 0.  Per Gaussian i
    weight_sum[i] = sum_{p participates, i blended at p} m(p) w_i(p)
    weight_max[i] = max_{p participates, i blended at p} w_i(p)           (0 where no such pixel exists)
    hits[i]       = #{p participates : i blended at p}
for ONE view (or band); the kernel accumulates into the caller's buffers, so statistics over several views are sums / maxima of these, and their budgets add
(weight_sum) or combine by max (weight_max).  Ambiguous pixels (BlendRef.ambiguous: float32 and float64 may decide the blended set differently there) leave
every comparison through m = 0 -- `participation(blend, m)` zeroes them, which is what participation is for.  The tests cap their share at 0.5 %.

The budgets (u = 2^-24, gamma as in gs_grad_ref)
-----------
weight_sum:  B_i = sum (gamma(n_p + 3) + Z_k) |m w| + gamma(n_acc) A_i + tiny_i,         A_i = sum |m w|
  n_p    blended entries of the pixel: the addend of entry k carries the roundings of T in front of it (T <- fmaf(-T, alpha, T): one per blended entry, <= n_p),
         the product w = alpha * T (1) and the product m * w (1); one more covers gamma's second-order terms.
  Z_k    the float32 error of alpha itself, BlendRef's Z(pixel, k) as gs_features_ref.py uses it for the map.
  n_acc  the additions a Gaussian's sum passes, each rounding a partial sum of magnitude <= A_i: the 4 DPP adds of the row reduction, at most 16 LDS float
         atomics (the tile's blocks) and one global float atomic per tile with a blending participant: n_acc = 4 + 16 + tiles_i.
  tiny_i = (2 sum max(1, |m|) + n_acc) 2^-126: a product below the normal range, or a subnormal partial sum, may be flushed.
  The relative part (B - tiny) / A is asserted <= gs_grad_ref.GATE (2e-3); A_i == 0 marks what must be EXACTLY zero (nothing is added to such a Gaussian).
weight_max:  |got - want| <= max over the participating blending pixels of (gamma(n_p + 2) + Z_k(p)) w_k(p)  (+ 2^-126)
  because |max f - max g| <= max |f - g| over a common index set, and the kernel's maximum adds no rounding to the colour's w (T chain: n_p, the product: 1,
  one more for the second order).  A = want: where no participating pixel blends i the value is exactly 0.
hits: exact.
"""
from __future__ import annotations

import numpy as np

from tests import gs_grad_ref as R

GATE = R.GATE
N_ROW, N_LDS = 4, 16


def participation(blend, m=None):
    """The (H, W) float32 map the kernel is handed: m (ones when None) with the ambiguous pixels zeroed (a copy)."""
    m = np.ones((blend.H, blend.W), np.float32) if m is None else np.array(m, np.float32, copy=True)
    assert m.shape == (blend.H, blend.W) and np.isfinite(m).all()
    m[blend.ambiguous] = 0
    return m


def random_map(blend, seed=0):
    """A non-negative (H, W) float32 map with exact zeros (about a quarter of the pixels) and a spread of magnitudes."""
    rng = np.random.default_rng(9000 + seed)
    m = (rng.random((blend.H, blend.W)) * np.exp(rng.normal(size=(blend.H, blend.W)))).astype(np.float32)
    m[rng.random((blend.H, blend.W)) < 0.25] = 0
    return m


class ContribRef:
    """One view: the three statistics of a BlendRef under the map m (already passed through `participation` when ambiguous pixels must leave), with budgets.
    Attributes (all (P,)): weight_sum, A, B, tiny, tiles; weight_max, B_max; hits (int64)."""

    def __init__(self, blend, m):
        m = np.asarray(m)
        assert m.dtype == np.float32 and m.shape == (blend.H, blend.W)
        P = blend.P
        f = np.float64
        self.weight_sum, self.A, rel, tiny = (np.zeros(P, f) for _ in range(4))
        self.weight_max, self.B_max = np.zeros(P, f), np.zeros(P, f)
        self.hits, self.tiles = np.zeros(P, np.int64), np.zeros(P, np.int64)
        for tl in blend.tiles:
            K, N = tl.al.shape
            mt = m[tl.py, tl.px].astype(f)
            part = mt != 0
            T = np.ones(N)
            rel_sum, rel_max = R.gamma(tl.n_p + 3), R.gamma(tl.n_p + 2)
            for k in range(K):
                a = tl.active[k]
                if not a.any():
                    continue
                w = tl.al[k] * T                                   # al is 0 where the pixel does not blend the entry
                T = T * (1.0 - tl.al[k])
                on = a & part
                if not on.any():
                    continue
                i = tl.ids[k]
                mw = np.abs(mt[on] * w[on])
                self.weight_sum[i] += (mt[on] * w[on]).sum()
                self.A[i] += mw.sum()
                rel[i] += ((rel_sum[on] + tl.Z[k][on]) * mw).sum()
                tiny[i] += 2 * np.maximum(1.0, np.abs(mt[on])).sum()
                self.weight_max[i] = max(self.weight_max[i], w[on].max())
                self.B_max[i] = max(self.B_max[i], ((rel_max[on] + tl.Z[k][on]) * w[on]).max())
                self.hits[i] += int(on.sum())
                self.tiles[i] += 1
        n_acc = N_ROW + N_LDS + self.tiles
        relp = rel + R.gamma(n_acc) * self.A
        assert (relp <= GATE * self.A).all(), 'the relative part of the weight_sum budget exceeds the 2e-3 gate'
        self.tiny = (tiny + n_acc) * R.TINY * (self.A > 0)
        self.B = relp + self.tiny
        assert (self.B_max <= GATE * self.weight_max).all()
        self.B_max = self.B_max + R.TINY * (self.weight_max > 0)


def brute_force(st, m):
    """The same three statistics by an independent per-pixel loop over a float64 forward state (points_xy, conic_opacity, point_list, ranges, n_contrib):
    no BlendRef, no vectorisation.  m (H, W).  Returns (weight_sum, weight_max, hits, T_final (H, W))."""
    W, H, P = int(st.W), int(st.H), int(st.P)
    gx = (W + 15) // 16
    pts, co = np.asarray(st.points_xy, np.float64), np.asarray(st.conic_opacity, np.float64)
    plist, ranges = np.asarray(st.point_list), np.asarray(st.ranges).astype(np.int64)
    ncon = np.asarray(st.n_contrib).astype(np.int64).reshape(H, W)
    ws, wm, hits, Tf = np.zeros(P), np.zeros(P), np.zeros(P, np.int64), np.ones((H, W))
    for y in range(H):
        for x in range(W):
            r0 = ranges[(y // 16) * gx + x // 16][0]
            T = 1.0
            for k in range(ncon[y, x]):
                i = plist[r0 + k]
                dx, dy = pts[i, 0] - x, pts[i, 1] - y
                power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
                if power > 0:
                    continue
                alpha = min(R.ALPHA_CAP, co[i, 3] * np.exp(power))
                if alpha < R.ALPHA_MIN:
                    continue
                w = alpha * T
                T = T * (1.0 - alpha)
                if m[y, x] != 0:
                    ws[i] += float(m[y, x]) * w
                    wm[i] = max(wm[i], w)
                    hits[i] += 1
            Tf[y, x] = T
    return ws, wm, hits, Tf
