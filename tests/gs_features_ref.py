"""A float64 restatement and a per-element error budget for the 3DGS feature pass (nerficg_amd/csrc/gs_features.hip: k_render_features, k_render_features_bw).
Plain module: no test functions.  Used by tests/test_gs_features_ref_cpu.py and tests/test_gpu_gs_features.py.

The statement
-------------
features (P, C) float32, promoted.  The blended set of a pixel, alpha, T and w = alpha T are BlendRef's (tests/gs_grad_ref.py): the list entries in front of
n_contrib with power <= 0 and alpha >= 1/255, in float64.  feature_map[c, p] = sum_i w_i(p) f[i, c], background 0.  The backward of L = <g, feature_map> is
BlendRef.sums run once per zero-padded TRIPLE of channels, with `rgb` replaced by the triple and bg = 0 -- exactly the ceil(C / 3) rasterizer calls with
colors_precomp triples that produce the same maps without the feature pass.  A run's colour columns are dL/df of its three channels; its six geometry columns
(opacity, mean2D x / y, conic xx / xy / yy) are that triple's share of the gradient through the weights, and the shares ADD (dL/dalpha is linear in the
channels).  LeafRef on the total gives every leaf.  Ambiguous pixels are BlendRef's (they do not depend on the features); the gradients are masked first.

The budget of the map (u = 2^-24, gamma as in gs_grad_ref)
---------------------
    B[c, p] = sum_k (gamma(2 n_p + 2) + Z_k) |w_k f_kc| + tiny,         A[c, p] = sum_k |w_k f_kc|
  n_p  blended entries of the pixel.  Entry k's term carries the roundings of T in front of it (T <- fmaf(-T, alpha, T): one per blended entry, <= n_p), the
       product w = alpha * T (1) and the fmaf that adds it (1); every later fmaf rounds the running sum, whose magnitude is at most A: n_p more.
  Z_k  the float32 error of alpha itself, as gs_grad_ref states it: BlendRef's Z(pixel, k) = sum_front alpha delta / (1 - alpha) + sum_{k and behind} delta / (1 - alpha)
       bounds what the map needs (the front entries through T, delta_k for alpha_k itself).
  tiny = n_p 2^-126: a product below the normal range may be flushed.
The relative part (B - tiny) / A is asserted <= 2e-3 (gs_grad_ref.GATE); A == 0 marks what must be exactly zero.

The budget of the backward
--------------------------
Per triple BlendRef.sums gives S, A, R, tiny with R = sum rel |addend|, rel = gamma(n_p + 4 cnt + C1) + Z, C1 = 24 counted on k_render_bw.  k_render_features_bw
walks the same chain (the forward's T, `r_om = rcp(1 - alpha_m); T_new = T * r_om`: 4 per step) and its statements differ from k_render_bw's in three places:
  * dL_dalpha is a chain of CH = 16 fmaf over the chunk's channels instead of 3 (+13), and has no background term (-5, not taken off);
  * the feature sums dchm * g_c are two products and four DPP adds from T (6 <= C1); the geometry sums pass four DPP adds as before;
  * accumulation is float32, not fixed point: a row's sum meets the tile's other blocks through LDS float atomics (at most 16 additions in any order), the
    flush multiplies a geometry sum by its constant (1) and adds it to the record with one global float atomic per (tile, chunk) (tiles x chunks additions); a
    feature element receives tiles additions (its own chunk only).  No truncation, so there is no `fixed` part.
    B_q = R_q + gamma(E + 1) A_q + gamma(n_acc) A_q + tiny_q      E = 13 (geometry; 0 for dL/df)      n_acc = chunks (tiles + 17) (geometry), tiles + 17 (dL/df)
gamma(E + 1) instead of a larger argument of rel's gamma: gamma(a + b) - gamma(a) <= gamma(b) / (1 - (a + b) u)^2, and the +1 covers that factor for every chain the
gate admits.  tiny_q = BlendRef's (eight products per addend) + n_acc 2^-126 (an atomic may flush a subnormal sum).  `tiles` is the largest over the triples
(a tile whose three gradient planes are all zero is skipped by that triple's run).
order='serial' (the float32 oracle, one thread, one run per triple): R + gamma(n_add) A + tiny per run, the runs' float32 results added in float64.
The relative part (B - tiny) / A is asserted <= 2e-3.

Colour and features together: the feature backward leaves its six sums in the records, then k_render_bw adds the colour's partial sums into them, one float
atomic per tile each of which rounds relative to a partial sum of magnitude <= A_colour + A_features:
    B = B_colour + B_features + gamma(tiles) A_features           (B_colour = gs_grad_ref.blend_budget, which already holds gamma(tiles + 2) A_colour)
"""
from __future__ import annotations

import copy

import numpy as np

from tests import gs_grad_ref as R

CH = 16
E_DALPHA = CH - 3
GATE = R.GATE


def _with_channels(blend, ch3):
    """`blend` with the three blended channels replaced by ch3 (P, 3) float64 and bg = 0 (a shallow copy: the geometry is shared)."""
    b = copy.copy(blend)
    b.bg, b.aux, b.tiles = np.zeros(3), False, []
    for tl in blend.tiles:
        t2 = copy.copy(tl)
        t2.c = ch3[tl.ids]
        b.tiles.append(t2)
    return b


class FeatureRef:
    """features (P, C) float32 on a BlendRef's decisions: `feature_map()` and `sums(g)`."""

    def __init__(self, blend, features):
        features = np.asarray(features)
        assert features.dtype == np.float32 and features.ndim == 2 and features.shape[0] == blend.P
        self.blend, self.C = blend, int(features.shape[1])
        self.n_triples = (self.C + 2) // 3
        f = np.zeros((blend.P, 3 * self.n_triples))
        f[:, :self.C] = features
        self.f = f
        self.chunks = (self.C + CH - 1) // CH

    def mask_ambiguous(self, g):
        return self.blend.mask_ambiguous(g)

    def feature_map(self):
        """(want, budget, A), each (C, H, W) float64."""
        b = self.blend
        want, bud, mag = (np.zeros((self.C, b.H, b.W)) for _ in range(3))
        for tl in b.tiles:
            K, N = tl.al.shape
            T = np.ones(N)
            acc, acc_b, acc_a = (np.zeros((self.C, N)) for _ in range(3))
            rel0 = R.gamma(2 * tl.n_p + 2)
            for k in range(K):
                a = tl.active[k]
                if not a.any():
                    continue
                w = tl.al[k] * T                                       # al is 0 where the pixel does not blend the entry
                term = self.f[tl.ids[k], :self.C, None] * w[None, :]
                acc += term
                acc_a += np.abs(term)
                acc_b += np.abs(term) * (rel0 + tl.Z[k])[None, :]
                T = T * (1.0 - tl.al[k])
            want[:, tl.py, tl.px], mag[:, tl.py, tl.px] = acc, acc_a
            assert (acc_b <= GATE * acc_a).all(), 'the relative part of the map budget exceeds the 2e-3 gate'
            bud[:, tl.py, tl.px] = acc_b + (tl.n_p * R.TINY)[None, :] * (acc_a > 0)
        return want, bud, mag

    def sums(self, g):
        """g (C, H, W) float32, already masked.  Returns dict: S, A, R, tiny (P, 9) with the colour columns zero and the six geometry columns summed over the
        triples; SF, AF, RF, tinyF (P, C) the feature gradient; tiles, n_add (P,) the largest over the triples; runs = BlendRef.sums' dict per triple."""
        g = np.asarray(g)
        b = self.blend
        assert g.dtype == np.float32 and g.shape == (self.C, b.H, b.W)
        P = b.P
        out = {k: np.zeros((P, 9)) for k in ('S', 'A', 'R', 'tiny')}
        out.update({k + 'F': np.zeros((P, 3 * self.n_triples)) for k in ('S', 'A', 'R', 'tiny')})
        out['tiles'], out['n_add'], out['runs'] = np.zeros(P, np.int64), np.zeros(P, np.int64), []
        for t in range(self.n_triples):
            g3 = np.zeros((3, b.H, b.W), np.float32)
            n = min(3, self.C - 3 * t)
            g3[:n] = g[3 * t:3 * t + n]
            run = _with_channels(b, self.f[:, 3 * t:3 * t + 3]).sums(g3)
            out['runs'].append(run)
            for k in ('S', 'A', 'R', 'tiny'):
                out[k][:, 3:] += run[k][:, 3:9]
                out[k + 'F'][:, 3 * t:3 * t + 3] = run[k][:, :3]
            out['tiles'] = np.maximum(out['tiles'], run['tiles'])
            out['n_add'] = np.maximum(out['n_add'], run['n_add'])
        for k in ('S', 'A', 'R', 'tiny'):
            out[k + 'F'] = out[k + 'F'][:, :self.C]
        out['chunks'] = self.chunks
        return out


def budget(ref, order='kernel'):
    """(B (P, 9), BF (P, C)) of the docstring from FeatureRef.sums' dict."""
    A, AF = ref['A'], ref['AF']
    if order == 'serial':
        B, BF = np.zeros_like(A), np.zeros_like(AF)
        for t, run in enumerate(ref['runs']):
            Bt = run['R'] + R.gamma(run['n_add'])[:, None] * run['A'] + run['tiny']
            B[:, 3:] += Bt[:, 3:9]
            n = min(3, AF.shape[1] - 3 * t)
            BF[:, 3 * t:3 * t + n] = Bt[:, :n]
        tiny, tinyF = ref['tiny'], ref['tinyF']
    else:
        n_acc = ref['tiles'] + 17
        tiny = ref['tiny'] + (ref['chunks'] * n_acc * R.TINY)[:, None] * (A > 0)
        tinyF = ref['tinyF'] + (n_acc * R.TINY)[:, None] * (AF > 0)
        B = ref['R'] + (R.gamma(E_DALPHA + 1) + R.gamma(ref['chunks'] * n_acc)[:, None]) * A + tiny
        BF = ref['RF'] + (R.gamma(1) + R.gamma(n_acc)[:, None]) * AF + tinyF
    assert (B - tiny <= GATE * A).all() and (BF - tinyF <= GATE * AF).all(), 'the relative part of the budget exceeds the 2e-3 gate'
    return B, BF


def combined(ref_f, B_f, ref_c, B_c):
    """Colour and features in one backward: (ref, B) for LeafRef -- the sums, magnitudes and budgets of the two passes as the docstring adds them."""
    tiles = np.maximum(ref_f['tiles'], ref_c['tiles'])
    ref = dict(S=ref_c['S'][:, :9] + ref_f['S'], A=ref_c['A'][:, :9] + ref_f['A'])
    return ref, B_c[:, :9] + B_f + R.gamma(tiles)[:, None] * ref_f['A']


def leaves(c, st64, ref, B):
    """gs_grad_ref.LeafRef on (P, 9) sums and budgets, chained to the raw parameters for a raw case (the tail of gs_grad_cases.reference_for)."""
    leaf = R.LeafRef(st64, ref, B)
    if c.form == 'raw':
        leaf.to_raw_parameters(st64.conic_opacity[:, 3], c.sc['scales'], c.sc['rotations'], np.sqrt((np.asarray(c.sc['raw']['quat'], np.float64) ** 2).sum(1)))
    return leaf


def random_features(P, C, seed=0):
    return np.random.default_rng(4000 + seed).normal(size=(P, C)).astype(np.float32)


def random_map_gradients(c, C, kind='normal', seed=0):
    """(C, H, W) float32 pixel gradients of a case in gs_grad_cases' kinds: the colour generator's planes, three at a time."""
    from tests import gs_grad_cases as GC
    planes = [GC.pixel_gradients(c, seed=7000 + seed + t, kind=kind)[0] for t in range((C + 2) // 3)]
    return np.ascontiguousarray(np.concatenate(planes)[:C])
