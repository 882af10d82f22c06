"""Float64 statements of the training compositor, the fused compositing + colour loss, the distortion loss, the inference compositor and the ray
gradients of the training march; a first-order f32 error budget for every output element; an np.float32 emulation of the wave-wide kernels with
wrong variants; the synthetic cases.  Plain module: no test functions.  Used by tests/test_train_composite_ref_cpu.py and
tests/test_gpu_train_composite.py.  U, SAFETY, EXPF_ULPS, EXP2_ULPS and ulp_f32 come from tests/image_composite_ref.py.

What is stated (from the reference's semantics, not from the kernels)
---------------------------------------------------------------------
  * volumerendering.cu:6-45 -- per row (ray_idx, start, N) of rays_a: a = 1 - exp(-sigma delta), w = a T, sums of w c, w t, w, then
    T <- T (1 - a).  The sample that brings T <= T_threshold is composited and the ray stops; total_samples is the index of that sample (it is
    composited but not counted) and N if the ray never stops.  ws is 0 behind the stop and in samples no ray owns; results land in slot ray_idx.
  * volumerendering.cu:87-151 -- the gradients of that forward with respect to sigma and the sample colours for upstream dL_dopacity,
    dL_ddepth, dL_drgb, dL_dws.  Stated here as torch.float64 autograd on the CPU through the forward statement, rays x K_max dense with a mask,
    the truncation held fixed.  The closed form (`closed_form_bw`) is a second voice only.  A sample with sigma = inf (delta > 0) has a = 1 and
    da/dsigma = delta exp(-sigma delta) -> 0: its gradient is the limit of the finite ones, delta * (the bracket of the closed form), in which
    every term carries the factor T_after = 0 or a suffix sum that is empty at a stopping sample.  Autograd reaches the same value through
    0 * delta; where it would yield NaN (0 * inf) the limit 0 is stated instead (`_autograd_bw`).
  * Renderer.py:78-84, Loss.py:15-22 -- the fused loss: the same forward, the pixel rgb + (1 - O) bg, alpha O, depth D / (O + 1e-6), the mean
    squared error over the 3 n_live colour values of the rows with ray_idx < counter[1], times the scale, and autograd back to dL/dsigma,
    dL/drgb.  Rows at or beyond n_live contribute nothing and get zero gradients.
  * losses.cu:9-61, :112-142 -- the distortion loss by its definition, sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 delta_i, evaluated directly
    in O(N^2) per ray on sorted ts; its gradient with respect to ws by float64 autograd; the inclusive scans ws_incl and wts_incl.
  * volumerendering.cu:205-249 -- inference compositing in place: the carry starts at 1 - opacity[r], the first n_eff samples of a row are
    used, alive <- -1 when n_eff == 0 and when the ray stops on T <= T_threshold.
  * custom_functions.py:122-137 -- dL/do = sum_i g_x_i, dL/dd = sum_i (t_i g_x_i + g_dir_i) per row, g_dirs optional.

The budgets
-----------
First-order bounds of the f32 rounding error, in float64, from the inputs alone, times SAFETY; one per output element, none exempt.
u = 2^-24, |delta| <= u |result| per rounding.  Per sample, x = sigma delta, e = exp(-x), a = 1 - e:
    x        one rounding: u relative
    e        the fast exponential exp2(x log2 e): e |x| (u + 2 u) for the argument (x's rounding, the rounded product, log2 e held as f32) plus
             EXP2_ULPS ulp of e.  x == 0: e = 1 exactly.  x = inf: e = 0 exactly.  An f32 result below 2^-126 may be flushed to zero: e below
             that is charged 2^-126 absolute.
    a        1 - e: exact for e >= 1/2 (Sterbenz), else u a.     1 - a: exact, it carries a's error.
    T        a product of the (1 - a): the kernels' products and sums are tree-ordered, so a product or a sum of n terms is charged n roundings
             relative to the sum (product) of the absolute terms -- n - 1 operations in ANY association, each rounding a partial result that is
             no larger than the whole.  The serial recurrence e_T' = e_T (1 - a) + T e_a + u T' charges exactly that (a factor that is exactly 1
             rounds nothing in any association either).  The scan shape of the kernels is not encoded.
    w        a T: e_w = e_a T + a e_T + u w
    sums     O, D, rgb over the n composited samples: sum of the terms' data errors (e_w |c| + u |w c| for a product term) + n u sum |term|.
A fused multiply-add rounds once where two roundings are charged: the bound covers contraction on and off.
dL/dsigma_k = delta_k [ sum_c g_c (c_k T_k' - (R_c - r_c)) + g_O (1 - O) + g_D (t_k T_k' - (D - d)) + T_k' g_w - (S - sc) ] with T_k' the
transmittance after sample k, r / d / sc the inclusive prefixes and S = sum dL_dws ws.  Charged: both operands of every R - r, D - d, S - sc
(the saved ray sum R, D, O at the rounding of the f32 value the test passes in, or at its own forward bound where the kernel recomputes it; the
recomputed prefix at its accumulated bound; S and sc on the f32 ws the test passes in: one rounding of ws, one of the product, n of the sum),
the rounding of each difference and product, 7 roundings of the bracket relative to the sum of its absolute terms, the product with delta.
dL/drgb_k = g w: e_w |g| + u |g w|.  Where the upstream gradient itself is computed (the fused loss) its bound e_g enters times the term.
The distortion forward is charged for the prefix form of losses.cu, 2 (wts_i w_excl - w_i wts_excl) + w_i^2 delta_i / 3: the scans at n roundings
of their absolute terms (w t: one more), both products and their difference, the constant 1/3 and three products, the per-sample additions and
n roundings of the ray's sum.  Its cancellation is real.  The backward the same way on t ws_incl[s-1] - wts_incl[s-1] and the two suffix
differences; the scans enter at one rounding (the f64 scans the test passes in, rounded) or at their forward bound (DistortionLoss.apply).
The inference compositor: T0 = 1 - opacity at one rounding, the walk as above; the value already in the output is one more term of the sum (the
reference adds every sample into it: n + 1 roundings of it too), one more rounding for `out += sum`.
The march backward: n roundings of sum |g_x|; t g_x one rounding each and 2 n roundings of sum (|t g_x| + |g_dir|).
The fused loss: pixel = R + (1 - O) bg: e_R + |bg| (e_O + u |1 - O|) + u |(1 - O) bg| + u |pixel|; depth = D / (O + 1e-6): the f32 constant 1e-6f
(u 1e-6), the sum, the quotient; squared error per ray and its sum over the rays (n_rays roundings), the division by 3 n_live, the scale; the
pixel gradient 2 / (3 n_live) (pixel - target) scale at three roundings, g_O = -(g . bg) at three products and three sums.

Threshold rays.  A ray whose T after some sample lies within SAFETY * e_T of T_threshold may stop one sample apart in f32.  The ray's LAST
sample counts too here (total_samples and `alive` depend on it).  An exact comparison (e_T = 0) is no threshold ray.  Every case keeps ZERO
threshold rays (asserted on the CPU from the f64 reference alone); SEEDS are chosen to meet it.  With none, total_samples, `alive` and the
support of ws and of both gradients must match the reference exactly.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests.image_composite_ref import EXP2_ULPS, EXPF_ULPS, SAFETY, U, ulp_f32  # noqa: F401  (EXPF_ULPS: sigma is an input here, no expf)

TINY = 2.0 ** -126
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1024)
N_RAYS = 45
K_MAX = 1024
# seeds for which the f64 reference alone meets the cases' conditions (zero threshold rays, the stop positions of `stops`, no stop in `thr0`):
# tests/test_train_composite_ref_cpu.py asserts them
SEEDS = dict(plain=21, stops=22, thr0=23, tie=24, extremes=25, inference=26, fused=27, march=28)
# (length, index of the constructed stop) of `stops`: indices 0, 63, 64, 65, >= 128 and the ray's own last sample, each at least once
STOP_PLAN = ((1, 0), (2, 0), (1024, 0), (64, 63), (127, 63), (65, 64), (128, 64), (129, 65), (300, 65), (129, 128), (300, 200), (1024, 640),
             (1024, 1023), (128, 127), (63, 62))
INFERENCE_N = (1, 3, 8, 33, 64, 65, 130)
FUSED = dict(n_live=37, scale=128.0, bg=(0.2, 0.5, 0.7), zero_a=600, zero_b=300, extra_capacity=100)
# largest budget on `plain` relative to the ray's largest |value| (printed by test_train_composite_ref_cpu.py from the reference alone); the CPU
# test asserts that the figures do not exceed these by more than 2x
PLAIN_CEILINGS = dict(ws=3.11e-5, opacity=8.10e-5, rgb=8.02e-5, depth=9.00e-5, dsigma=1.78e-4, drgb=3.12e-5)


# ------------------------------------------------------------------------------------------------ layout
def dense_index(rays_a, K):
    """(idx, mask) of shape (rows, K): idx[n, k] = start_n + k where k < N_n (0 elsewhere)."""
    rays_a = np.asarray(rays_a, np.int64)
    k = np.arange(K)[None, :]
    mask = k < rays_a[:, 2:3]
    return np.where(mask, rays_a[:, 1:2] + k, 0), mask


def to_dense(flat, idx, mask):
    v = np.asarray(flat, np.float64)[idx]
    m = mask if v.ndim == 2 else mask[..., None]
    return np.where(m, v, 0.0)


def to_flat(dense, idx, mask, M):
    out = np.zeros((M,) + dense.shape[2:], np.float64)
    out[idx[mask]] = dense[mask]
    return out


# ------------------------------------------------------------------------------------------------ the forward walk and its budget
def _walk(sig, rgbs, dl, ts, N, thr, T0=None, e_T0=None):
    """Front to back over dense (R, K) float64 samples, vectorised over the rays: the reference values and the first-order error terms of the
    module docstring (without SAFETY).  T0 / e_T0: the transmittance a ray starts with (inference) and its bound."""
    u = U
    R, K = sig.shape
    N = np.asarray(N, np.int64)
    thr = float(np.float32(thr))
    T = np.ones(R) if T0 is None else np.array(T0, np.float64)
    e_T = np.zeros(R) if e_T0 is None else np.array(e_T0, np.float64)
    z = lambda: np.zeros((R, K))
    out = dict(a=z(), e_a=z(), Tb=z(), Ta=z(), e_Ta=z(), w=z(), e_w=z(), comp=np.zeros((R, K), bool))
    alive = N > 0
    stop = np.full(R, -1, np.int64)
    threshold = np.zeros(R, bool)
    for k in range(int(N.max(initial=0))):
        act = alive & (k < N)
        if not act.any():
            break
        with np.errstate(over='ignore', invalid='ignore'):
            x = np.where(act, sig[:, k] * dl[:, k], 0.0)
            e = np.exp(-x)
            a = -np.expm1(-x)
            xf = np.where(np.isfinite(x), x, 0.0)
            e_e = np.where((x == 0) | ~np.isfinite(x), 0.0, e * xf * 3 * u + EXP2_ULPS * ulp_f32(e) + np.where(e < TINY, TINY, 0.0))
            e_a = e_e + np.where(e >= 0.5, 0.0, u * a)
            w = a * T
            e_w = e_a * T + a * e_T + u * w
            T_new = T * e
            e_Tn = e_T * e + T * e_a + np.where(e == 1.0, 0.0, u * T_new)
        for key, v in (('a', a), ('e_a', e_a), ('Tb', T), ('Ta', T_new), ('e_Ta', e_Tn), ('w', w), ('e_w', e_w)):
            out[key][:, k] = np.where(act, v, 0.0)
        out['comp'][:, k] = act
        T, e_T = np.where(act, T_new, T), np.where(act, e_Tn, e_T)
        threshold |= act & (e_T > 0) & (np.abs(T - thr) <= SAFETY * e_T)
        stops = act & (T <= thr)
        stop = np.where(stops, k, stop)
        alive = alive & ~stops
    comp = out['comp']
    n = comp.sum(axis=1)
    w, e_w = out['w'], out['e_w']
    sums, errs = {}, {}
    for key, coef in (('opacity', np.ones_like(w)), ('depth', ts), ('r', rgbs[..., 0]), ('g', rgbs[..., 1]), ('b', rgbs[..., 2])):
        coef = np.where(comp, coef, 0.0)
        term = w * coef
        sums[key] = term.sum(axis=1)
        prod = 0.0 if key == 'opacity' else u * np.abs(term)
        errs[key] = (e_w * np.abs(coef) + prod).sum(axis=1) + n * u * np.abs(term).sum(axis=1)
    out.update(N=N, n=n, stop=stop, total=np.where(stop >= 0, stop, N), threshold=threshold, T=T, e_T=e_T, opacity=sums['opacity'], depth=sums['depth'],
               rgb=np.stack([sums['r'], sums['g'], sums['b']], axis=1), e_opacity=errs['opacity'], e_depth=errs['depth'],
               e_rgb=np.stack([errs['r'], errs['g'], errs['b']], axis=1))
    return out


def _prefix_terms(s, coef):
    """Inclusive prefix of w * coef over the composited samples and its accumulated bound (recomputed in f32 by the backward kernels)."""
    comp = s['comp']
    coef = np.where(comp, coef, 0.0)
    term = s['w'] * coef
    cnt = np.cumsum(comp, axis=1)
    pref = np.cumsum(term, axis=1)
    err = np.cumsum(s['e_w'] * np.abs(coef) + U * np.abs(term), axis=1) + cnt * U * np.cumsum(np.abs(term), axis=1)
    return pref, err


def closed_form_bw(s, rgbs, dl, ts, go, gd, gr, gw, e_sum=None, e_g=None, own_ws=False):
    """The closed form of volumerendering.cu:87-151 in float64 on the walk `s` (dense arrays; go, gd (R), gr (R, 3), gw (R, K) or None), and
    the budget of an f32 evaluation of it (module docstring; SAFETY not applied).  e_sum = (e_O, e_D, e_rgb): the bounds of the saved ray sums
    (default: the rounding of the f32 value passed in).  e_g = (e_gO, e_gD, e_gr): bounds of the upstream gradients (default: exact).
    own_ws: the ws handed in are an f32 forward's own (bound e_w) instead of the float64 ones rounded (u w).
    Returns dsigma, drgb (R, K, 3), e_dsigma, e_drgb and |delta| * (the sum of the bracket's absolute operands)."""
    u = U
    comp = s['comp']
    R_, K = comp.shape
    Ta, e_Ta, w, e_w = s['Ta'], s['e_Ta'], s['w'], s['e_w']
    O, D, RGB = s['opacity'], s['depth'], s['rgb']
    e_O, e_D, e_RGB = (u * np.abs(O), u * np.abs(D), u * np.abs(RGB)) if e_sum is None else e_sum
    e_gO, e_gD, e_gr = (np.zeros(R_), np.zeros(R_), np.zeros((R_, 3))) if e_g is None else e_g
    gd = np.zeros(R_) if gd is None else gd
    go = np.zeros(R_) if go is None else go
    gw = np.zeros((R_, K)) if gw is None else np.where(comp, gw, 0.0)
    terms, e_terms, operands = [], [], []

    def suffix_term(g, e_gup, coef, total, e_total):
        pref, e_pref = _prefix_terms(s, coef)
        coef = np.where(comp, coef, 0.0)
        diff = total[:, None] - pref
        inner = coef * Ta - diff
        e_inner = np.abs(coef) * e_Ta + u * np.abs(coef * Ta) + e_total[:, None] + e_pref + u * np.abs(diff) + u * np.abs(inner)
        t = g[:, None] * inner
        terms.append(t)
        operands.append(np.abs(g)[:, None] * (np.abs(coef * Ta) + np.abs(total)[:, None] + np.abs(pref)))
        e_terms.append(np.abs(g)[:, None] * e_inner + e_gup[:, None] * np.abs(inner) + u * np.abs(t))

    for c in range(3):
        suffix_term(gr[:, c], e_gr[:, c], rgbs[..., c], RGB[:, c], e_RGB[:, c])
    tO = go * (1 - O)
    terms.append(np.broadcast_to(tO[:, None], (R_, K)))
    operands.append(np.broadcast_to((np.abs(go) * (1 + np.abs(O)))[:, None], (R_, K)))
    e_terms.append(np.broadcast_to((np.abs(go) * (e_O + u * np.abs(1 - O)) + e_gO * np.abs(1 - O) + u * np.abs(tO))[:, None], (R_, K)))
    suffix_term(gd, e_gD, ts, D, e_D)
    tW = Ta * gw
    terms.append(tW)
    operands.append(np.abs(tW))
    e_terms.append(np.abs(gw) * e_Ta + u * np.abs(tW))
    # S - sc on the ws the caller passes in (w rounded to f32): per product one rounding of ws and one of the product; n roundings of the sums
    pw = gw * w
    S, sc = pw.sum(axis=1), np.cumsum(pw, axis=1)
    apw = np.abs(pw)
    e_pw = np.abs(gw) * (e_w if own_ws else u * w) + u * apw
    e_S = e_pw.sum(axis=1) + s['N'] * u * apw.sum(axis=1)
    e_sc = np.cumsum(e_pw, axis=1) + np.cumsum(comp, axis=1) * u * np.cumsum(apw, axis=1)
    tS = S[:, None] - sc
    terms.append(-tS)
    operands.append(np.abs(S)[:, None] + np.abs(sc))
    e_terms.append(e_S[:, None] + e_sc + u * np.abs(tS))
    bracket = sum(terms)
    e_bracket = sum(e_terms) + len(terms) * u * sum(np.abs(t) for t in terms)
    dsig = np.where(comp, dl * bracket, 0.0)
    e_dsig = np.where(comp, np.abs(dl) * e_bracket + u * np.abs(dsig), 0.0)
    drgb = np.where(comp[..., None], gr[:, None, :] * w[..., None], 0.0)
    e_drgb = np.where(comp[..., None], np.abs(gr)[:, None, :] * e_w[..., None] + e_gr[:, None, :] * w[..., None] + u * np.abs(drgb), 0.0)
    scale = np.where(comp, np.abs(dl) * sum(operands), 0.0)      # what the float64 closed form itself subtracts: its own rounding scale
    return dsig, drgb, e_dsig, e_drgb, scale


def _torch_forward(sig, rgbs, dl, ts, comp):
    """The forward statement in torch.float64 on dense (R, K) samples, the truncation `comp` held fixed.  Returns O, D, RGB (R, 3), ws (R, K)."""
    x = sig * dl
    e = torch.where(comp, torch.exp(-x), torch.ones_like(x))
    a = torch.where(comp, -torch.expm1(-x), torch.zeros_like(x))
    T_after = torch.cumprod(e, dim=1)
    T_before = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], dim=1)
    w = a * T_before
    return w.sum(1), (w * ts).sum(1), (w[..., None] * rgbs).sum(1), w


def _autograd_bw(sig, rgbs, dl, ts, comp, loss_of):
    """dL/dsigma, dL/drgbs (dense, float64) of loss_of(O, D, RGB, ws) by autograd.  Samples outside `comp` get 0.  A non-finite sigma whose
    gradient autograd cannot form (NaN out of 0 * inf) gets the limit 0 (module docstring)."""
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    sig_t = T(np.where(comp, sig, 0.0)).requires_grad_()
    rgb_t = T(np.where(comp[..., None], rgbs, 0.0)).requires_grad_()
    loss = loss_of(*_torch_forward(sig_t, rgb_t, T(np.where(comp, dl, 0.0)), T(np.where(comp, ts, 0.0)), T(comp)))
    loss.backward()
    ds, dr = sig_t.grad.numpy().copy(), rgb_t.grad.numpy().copy()
    ds = np.where(~np.isfinite(sig) & np.isnan(ds), 0.0, ds)
    return np.where(comp, ds, 0.0), np.where(comp[..., None], dr, 0.0)


# ------------------------------------------------------------------------------------------------ the train compositor on a case
def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _ro(v)
    return d


def _dense_case(case):
    idx, mask = dense_index(case['rays_a'], K_MAX)
    d = dict(idx=idx, mask=mask, N=case['rays_a'][:, 2].astype(np.int64), ray_idx=case['rays_a'][:, 0].astype(np.int64))
    for key in ('sigmas', 'rgbs', 'deltas', 'ts', 'gw'):
        d[key] = to_dense(case[key], idx, mask)
    return d


def train_reference_of(case, null_grads=False):
    """Forward and backward float64 reference of a case with every budget (SAFETY applied).  Per-ray outputs are in SLOT order (ray_idx),
    per-sample outputs flat (M).  null_grads: dL_dopacity, dL_ddepth and dL_dws absent (zero)."""
    d = _dense_case(case)
    idx, mask, slot = d['idx'], d['mask'], d['ray_idx']
    M, n = case['sigmas'].shape[0], len(slot)
    s = _walk(d['sigmas'], d['rgbs'], d['deltas'], d['ts'], d['N'], case['T_threshold'])
    go, gd, gr = (case[k].astype(np.float64)[slot] for k in ('go', 'gd', 'gr'))
    gw = d['gw']
    if null_grads:
        go, gd, gw = np.zeros(n), np.zeros(n), np.zeros_like(gw)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    loss_of = lambda O, D, RGB, ws: (O * T(go)).sum() + (D * T(gd)).sum() + (RGB * T(gr)).sum() + (ws * T(np.where(s['comp'], gw, 0.0))).sum()
    ds, dr = _autograd_bw(d['sigmas'], d['rgbs'], d['deltas'], d['ts'], s['comp'], loss_of)
    cds, cdr, e_ds, e_dr, c_scale = closed_form_bw(s, d['rgbs'], d['deltas'], d['ts'], go, gd, gr, gw)

    def by_slot(v):
        out = np.zeros((n,) + v.shape[1:], v.dtype)
        out[slot] = v
        return out
    flat = lambda v: to_flat(v, idx, mask, M)
    owner = np.full(M, -1, np.int64)
    owner[idx[mask]] = np.nonzero(mask)[0]
    ref = dict(total=by_slot(s['total']), opacity=by_slot(s['opacity']), depth=by_slot(s['depth']), rgb=by_slot(s['rgb']), ws=flat(s['w']),
               dsigma=flat(ds), drgb=flat(dr), closed_dsigma=flat(cds), closed_drgb=flat(cdr), closed_operands=flat(c_scale),
               support=flat(s['comp'].astype(np.float64)) > 0, threshold=s['threshold'], stop=s['stop'], N=d['N'], owner=owner, row_of_slot=np.argsort(slot),
               budget=dict(opacity=SAFETY * by_slot(s['e_opacity']), depth=SAFETY * by_slot(s['e_depth']), rgb=SAFETY * by_slot(s['e_rgb']),
                           ws=SAFETY * flat(s['e_w']), dsigma=SAFETY * flat(e_ds), drgb=SAFETY * flat(e_dr)))
    return _ro(ref)


@functools.lru_cache(maxsize=None)
def train_reference(name, null_grads=False):
    return train_reference_of(cases()[name], null_grads)


@functools.lru_cache(maxsize=None)
def train_reference_own_sums(name):
    """{'dsigma', 'drgb'}: the backward budgets (flat, SAFETY applied) when the backward is handed an f32 forward's OWN ws, opacity, depth and rgb
    (VolumeRenderer.apply) instead of the float64 ones rounded: each enters at its forward bound."""
    case = cases()[name]
    d = _dense_case(case)
    slot = d['ray_idx']
    s = _walk(d['sigmas'], d['rgbs'], d['deltas'], d['ts'], d['N'], case['T_threshold'])
    go, gd, gr = (case[k].astype(np.float64)[slot] for k in ('go', 'gd', 'gr'))
    _, _, e_ds, e_dr, _ = closed_form_bw(s, d['rgbs'], d['deltas'], d['ts'], go, gd, gr, d['gw'], e_sum=(s['e_opacity'], s['e_depth'], s['e_rgb']), own_ws=True)
    M = case['sigmas'].shape[0]
    return _ro(dict(dsigma=SAFETY * to_flat(e_ds, d['idx'], d['mask'], M), drgb=SAFETY * to_flat(e_dr, d['idx'], d['mask'], M)))


# ------------------------------------------------------------------------------------------------ the fused loss
@functools.lru_cache(maxsize=None)
def fused_case():
    """The samples of `stops` as one fused training iteration: 45 rows of capacity, 37 live, counter[0] = the samples in use, below the capacity."""
    base = cases()['stops']
    rng = np.random.default_rng(SEEDS['fused'])
    M = base['sigmas'].shape[0]
    case = dict(base)
    case.update(FUSED)
    case.update(target=rng.random((N_RAYS, 3)).astype(np.float32), counter=np.array([M, FUSED['n_live']], np.int32), ray_capacity=N_RAYS,
                sample_capacity=M + FUSED['extra_capacity'])
    return _ro(case)


@functools.lru_cache(maxsize=None)
def fused_reference():
    case = fused_case()
    u = U
    d = _dense_case(case)
    idx, mask, slot = d['idx'], d['mask'], d['ray_idx']
    n, M = len(slot), case['sigmas'].shape[0]
    n_live, scale = case['n_live'], float(case['scale'])
    bg = np.asarray(case['bg'], np.float32).astype(np.float64)
    target = case['target'].astype(np.float64)[slot]
    live = slot < n_live
    s = _walk(d['sigmas'], d['rgbs'], d['deltas'], d['ts'], d['N'], case['T_threshold'])
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))

    def loss_of(O, D, RGB, ws):
        pix = RGB + (1 - O)[:, None] * T(bg)
        return ((pix - T(target)) ** 2 * T(live.astype(np.float64))[:, None]).sum() / (3 * n_live) * scale
    ds, dr = _autograd_bw(d['sigmas'], d['rgbs'], d['deltas'], d['ts'], s['comp'], loss_of)
    O, D, RGB = s['opacity'], s['depth'], s['rgb']
    e_O, e_D, e_RGB = s['e_opacity'], s['e_depth'], s['e_rgb']
    see = 1 - O
    pix = RGB + see[:, None] * bg
    e_pix = e_RGB + (e_O + u * np.abs(see))[:, None] * np.abs(bg) + u * np.abs(see[:, None] * bg) + u * np.abs(pix)
    den = O + 1e-6
    e_den = e_O + u * 1e-6 + u * den
    depth = D / den
    with np.errstate(divide='ignore', invalid='ignore'):
        e_depth = np.where(den > 2 * SAFETY * e_den, (e_D + np.abs(depth) * e_den) / (den - SAFETY * e_den) + u * np.abs(depth), np.inf)
    e_depth = np.where(d['N'] > 0, e_depth, 0.0)       # a ray without samples: 0 / 1e-6, exactly 0
    diff = np.where(live[:, None], pix - target, 0.0)
    e_diff = np.where(live[:, None], e_pix + u * np.abs(diff), 0.0)
    sq = (diff ** 2).sum(axis=1)
    e_sq = (2 * np.abs(diff) * e_diff + u * diff ** 2).sum(axis=1) + 3 * u * sq
    tot = sq.sum()
    mean = tot / (3 * n_live)
    e_mean = (e_sq.sum() + n * u * tot) / (3 * n_live) + u * mean
    k = 2.0 / (3 * n_live) * scale
    g = k * diff
    e_g = k * e_diff + 3 * u * np.abs(g)
    gO = -(g * bg).sum(axis=1)
    e_gO = (e_g * np.abs(bg) + u * np.abs(g * bg)).sum(axis=1) + 3 * u * np.abs(g * bg).sum(axis=1)
    cds, cdr, e_ds, e_dr, _ = closed_form_bw(s, d['rgbs'], d['deltas'], d['ts'], gO, None, g, None, e_sum=(e_O, e_D, e_RGB),
                                             e_g=(e_gO, np.zeros(n), e_g))

    def by_slot(v):
        out = np.zeros((n,) + v.shape[1:], v.dtype)
        out[slot] = v
        return out
    flat = lambda v: to_flat(v, idx, mask, M)
    owner = np.full(M, -1, np.int64)
    owner[idx[mask]] = np.nonzero(mask)[0]
    dead_samples = np.zeros(M, bool)
    dead_samples[idx[mask & ~live[:, None]]] = True
    ref = dict(pixel=by_slot(pix), alpha=by_slot(O), depth=by_slot(depth), loss2=np.array([mean, mean * scale]), dsigma=flat(ds), drgb=flat(dr),
               closed_dsigma=flat(cds), closed_drgb=flat(cdr), support=flat(s['comp'].astype(np.float64)) > 0, owned=owner >= 0, owner=owner,
               dead_samples=dead_samples, threshold=s['threshold'], row_of_slot=np.argsort(slot),
               budget=dict(pixel=SAFETY * by_slot(e_pix), alpha=SAFETY * by_slot(e_O), depth=SAFETY * by_slot(e_depth),
                           loss2=SAFETY * np.array([e_mean, e_mean * scale + u * mean * scale]), dsigma=SAFETY * flat(e_ds), drgb=SAFETY * flat(e_dr)))
    return _ro(ref)


# ------------------------------------------------------------------------------------------------ the distortion loss
def distortion_reference_of(ws, deltas, ts, rays_a, g_loss, scans='rounded'):
    """Definition (O(N^2) per ray), float64 autograd for dL/dws with upstream g_loss (per slot), the inclusive scans, and the budgets.
    scans: how the backward's scan inputs come in -- 'rounded' (the float64 scans rounded to f32) or 'computed' (their forward bound)."""
    u = U
    rays_a = np.asarray(rays_a, np.int64)
    idx, mask = dense_index(rays_a, K_MAX)
    slot, N = rays_a[:, 0], rays_a[:, 2]
    n, M = len(slot), ws.shape[0]
    w, dl, t = (to_dense(v, idx, mask) for v in (ws, deltas, ts))
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    w_t = T(w).requires_grad_()
    t_t, dl_t = T(t), T(dl)
    pair = lambda wr, tr: (wr[None, :] * wr[:, None] * (tr[None, :] - tr[:, None]).abs()).sum()
    loss_t = torch.stack([pair(w_t[r, :int(N[r])], t_t[r, :int(N[r])]) for r in range(n)])
    loss_t = loss_t + (w_t ** 2 * dl_t).sum(1) / 3
    g = np.asarray(g_loss, np.float64)[slot]
    (loss_t * T(g)).sum().backward()
    dws = np.where(mask, w_t.grad.numpy(), 0.0)
    loss = loss_t.detach().numpy()
    # scans and the prefix form of losses.cu
    cnt = np.cumsum(mask, axis=1)
    wt = w * t
    wi, wti = np.cumsum(w, axis=1), np.cumsum(wt, axis=1)
    e_wi = cnt * u * np.cumsum(np.abs(w), axis=1)
    e_wti = np.cumsum(u * np.abs(wt), axis=1) + cnt * u * np.cumsum(np.abs(wt), axis=1)
    shift = lambda v: np.concatenate([np.zeros((n, 1)), v[:, :-1]], axis=1)
    we, wte, e_we, e_wte = shift(wi), shift(wti), shift(e_wi), shift(e_wti)
    p1, p2 = wti * we, wi * wte
    e_p = e_wti * np.abs(we) + np.abs(wti) * e_we + u * np.abs(p1) + e_wi * np.abs(wte) + np.abs(wi) * e_wte + u * np.abs(p2)
    cross = 2 * (p1 - p2)
    third = w * w * dl / 3
    l = cross + third
    e_l = 2 * (e_p + u * np.abs(p1 - p2)) + 4 * u * np.abs(third) + u * np.abs(l) + u * np.abs(l)      # the sum of the two, and `acc +=`
    e_l, l = np.where(mask, e_l, 0.0), np.where(mask, l, 0.0)
    e_loss = e_l.sum(axis=1) + N * u * np.abs(l).sum(axis=1)
    # backward on the scans it is handed
    if scans == 'rounded':
        e_wi_in, e_wti_in = u * np.abs(wi), u * np.abs(wti)
    else:
        e_wi_in, e_wti_in = e_wi, e_wti
    last = np.maximum(N - 1, 0)
    rows = np.arange(n)
    ws_sum, wts_sum = wi[rows, last], wti[rows, last]
    e_ws_sum, e_wts_sum = e_wi_in[rows, last], e_wti_in[rows, last]
    wi_p, wti_p, e_wi_p, e_wti_p = shift(wi), shift(wti), shift(e_wi_in), shift(e_wti_in)
    prev = t * wi_p - wti_p
    e_prev = np.abs(t) * e_wi_p + u * np.abs(t * wi_p) + e_wti_p + u * np.abs(prev)
    A = wts_sum[:, None] - wti
    e_A = e_wts_sum[:, None] + e_wti_in + u * np.abs(A)
    B = ws_sum[:, None] - wi
    e_B = e_ws_sum[:, None] + e_wi_in + u * np.abs(B)
    C = A - t * B
    e_C = e_A + np.abs(t) * e_B + u * np.abs(t * B) + u * np.abs(C)
    X = prev + C
    e_X = e_prev + e_C + u * np.abs(X)
    v1 = 2 * g[:, None] * X
    v2 = 2 * g[:, None] / 3 * w * dl
    e_dws = np.abs(2 * g)[:, None] * e_X + u * np.abs(v1) + 3 * u * np.abs(v2) + u * np.abs(v1 + v2)
    closed = np.where(mask, v1 + v2, 0.0)

    def by_slot(v):
        out = np.zeros(n)
        out[slot] = v
        return out
    flat = lambda v: to_flat(np.where(mask, v, 0.0), idx, mask, M)
    owner = np.full(M, -1, np.int64)
    owner[idx[mask]] = np.nonzero(mask)[0]
    return _ro(dict(loss=by_slot(loss), ws_incl=flat(wi), wts_incl=flat(wti), dws=flat(dws), closed_dws=flat(closed), owner=owner, N=N,
                    row_of_slot=np.argsort(slot),
                    budget=dict(loss=SAFETY * by_slot(e_loss), ws_incl=SAFETY * flat(e_wi), wts_incl=SAFETY * flat(e_wti), dws=SAFETY * flat(e_dws))))


@functools.lru_cache(maxsize=None)
def distortion_cases():
    """name -> dict(ws f32 (the reference ws of the train case, zeros behind the stops), deltas, ts, rays_a, g_loss)."""
    out = {}
    for name in ('plain', 'stops'):
        c = cases()[name]
        ws = train_reference(name)['ws'].astype(np.float32)
        g = np.random.default_rng(SEEDS[name] + 100).normal(size=N_RAYS).astype(np.float32)
        out[name] = _ro(dict(ws=ws, deltas=c['deltas'], ts=c['ts'], rays_a=c['rays_a'], g_loss=g))
    c = dict(out['plain'])
    with np.errstate(invalid='ignore'):
        c['ts'] = (np.floor(c['ts'] * np.float32(16)) / np.float32(16)).astype(np.float32)      # runs of equal positions, still sorted
    out['equal_ts'] = _ro(c)
    return out


@functools.lru_cache(maxsize=None)
def distortion_reference(name, scans='rounded'):
    c = distortion_cases()[name]
    return distortion_reference_of(c['ws'], c['deltas'], c['ts'], c['rays_a'], c['g_loss'], scans)


# ------------------------------------------------------------------------------------------------ inference compositing
@functools.lru_cache(maxsize=None)
def inference_case(n_samples):
    """100 rays, 70 of them alive (a permuted subset), rows of n_samples samples, n_eff from 0 to n_samples, starting opacities in [0, 0.9],
    half the rays dense enough to stop."""
    rng = np.random.default_rng(SEEDS['inference'] + n_samples)
    n_total, n_alive = 100, 70
    alive = rng.permutation(n_total)[:n_alive].astype(np.int64)
    n_eff = rng.integers(0, n_samples + 1, n_alive).astype(np.int32)
    n_eff[:4] = (0, n_samples, 0, n_samples)
    dl = rng.uniform(1e-3, 1.1e-2, (n_alive, n_samples)).astype(np.float32)
    sig = rng.uniform(0, 4, (n_alive, n_samples))
    dense_rays = rng.random(n_alive) < 0.5
    # a dense ray reaches T = 1e-4 / 3 at a drawn fraction of its samples
    x = sig * dl
    at = np.maximum((rng.uniform(0.2, 0.9, n_alive) * np.maximum(n_eff, 1)).astype(np.int64), 0)
    level = 10.3 / np.maximum(np.cumsum(x, axis=1)[np.arange(n_alive), np.minimum(at, n_samples - 1)], 1e-9)
    sig = np.where(dense_rays[:, None], sig * level[:, None], sig).astype(np.float32)
    # constructed stops (sigma delta = 20 behind thin samples) on whole rows: at the row's last sample, at sample 64 (or the last) and at sample 0
    for row, at in ((4, n_samples - 1), (5, min(64, n_samples - 1)), (6, 0)):
        n_eff[row], dense_rays[row] = n_samples, True
        sig[row, :at] = (rng.uniform(0, 2.0, at) / max(at, 1)).astype(np.float32) / dl[row, :at]
        sig[row, at] = np.float32(20.0) / dl[row, at]
    ts = (0.2 + np.cumsum(dl, axis=1)).astype(np.float32)
    opacity = np.where(rng.random(n_total) < 0.3, 0.0, rng.uniform(0, 0.9, n_total)).astype(np.float32)
    case = dict(sigmas=sig, rgbs=rng.random((n_alive, n_samples, 3)).astype(np.float32), deltas=dl, ts=ts, alive=alive, n_eff=n_eff, opacity=opacity,
                depth=(opacity * rng.uniform(0.2, 2, n_total)).astype(np.float32), rgb=(opacity[:, None] * rng.random((n_total, 3))).astype(np.float32),
                T_threshold=1e-4, n_samples=n_samples, dense_rays=dense_rays)
    return _ro(case)


@functools.lru_cache(maxsize=None)
def inference_reference(n_samples):
    c = inference_case(n_samples)
    u = U
    r = c['alive']
    O0 = c['opacity'].astype(np.float64)[r]
    T0 = 1 - O0
    e_T0 = np.where(O0 == 0, 0.0, u * T0)
    N = c['n_eff'].astype(np.int64)
    s = _walk(c['sigmas'].astype(np.float64), c['rgbs'].astype(np.float64), c['deltas'].astype(np.float64), c['ts'].astype(np.float64), N,
              c['T_threshold'], T0, e_T0)
    out, bud = {}, {}
    for key, add, e_add in (('opacity', s['opacity'], s['e_opacity']), ('depth', s['depth'], s['e_depth']), ('rgb', s['rgb'], s['e_rgb'])):
        v = c[key].astype(np.float64).copy()
        b = np.zeros_like(v)
        v[r] = v[r] + add
        used = (N > 0) if add.ndim == 1 else (N > 0)[:, None]
        n1 = (s['n'] + 1) if add.ndim == 1 else (s['n'] + 1)[:, None]
        b[r] = np.where(used, e_add + n1 * u * np.abs(c[key].astype(np.float64)[r]) + u * np.abs(v[r]), 0.0)
        out[key], bud[key] = v, SAFETY * b
    alive = np.where((N == 0) | (s['stop'] >= 0), -1, r)
    out.update(alive=alive, threshold=s['threshold'], stop=s['stop'], N=N, budget=bud)
    return _ro(out)


# ------------------------------------------------------------------------------------------------ ray gradients of the march
@functools.lru_cache(maxsize=None)
def march_case():
    base = cases()['plain']
    rng = np.random.default_rng(SEEDS['march'])
    M = base['ts'].shape[0]
    return _ro(dict(rays_a=base['rays_a'], ts=base['ts'], g_xyzs=rng.normal(size=(M, 3)).astype(np.float32), g_dirs=rng.normal(size=(M, 3)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def march_reference(with_dirs):
    """g_o, g_d per ROW of rays_a (custom_functions.py:122-137) and their budgets."""
    c = march_case()
    u = U
    idx, mask = dense_index(c['rays_a'], K_MAX)
    N = c['rays_a'][:, 2].astype(np.float64)
    gx = to_dense(c['g_xyzs'], idx, mask)
    gdir = to_dense(c['g_dirs'], idx, mask) if with_dirs else np.zeros_like(gx)
    t = to_dense(c['ts'], idx, mask)[..., None]
    g_o = gx.sum(axis=1)
    e_o = N[:, None] * u * np.abs(gx).sum(axis=1)
    g_d = (t * gx + gdir).sum(axis=1)
    e_d = (u * np.abs(t * gx)).sum(axis=1) + 2 * N[:, None] * u * (np.abs(t * gx) + np.abs(gdir)).sum(axis=1)
    return _ro(dict(g_o=g_o, g_d=g_d, N=c['rays_a'][:, 2], budget=dict(g_o=SAFETY * e_o, g_d=SAFETY * e_d)))


# ------------------------------------------------------------------------------------------------ the kernels' shape in np.float32
def _exp32(v):
    """exp of an f32 argument, evaluated in double and rounded once"""
    with np.errstate(over='ignore'):
        return np.exp(v.astype(np.float64)).astype(np.float32)


def _scan(v, op):
    """Inclusive doubling scan along axis 1 in the array's own precision (the shape of a wave-wide shuffle scan)."""
    d = 1
    while d < v.shape[1]:
        nv = v.copy()
        nv[:, d:] = op(v[:, d:], v[:, :-d])
        v, d = nv, d * 2
    return v


def _tree(v):
    """Butterfly sum along axis 1 (a power of two wide)."""
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = v[:, :h] + v[:, h:]
    return v[:, 0]


def _pad(v, K):
    out = np.zeros((v.shape[0], K) + v.shape[2:], v.dtype)
    out[:, :v.shape[1]] = v
    return out


def _chunk_T(a, carry, open_, mutant):
    f = np.float32
    incl = _scan(f(1) - a, np.multiply)
    excl = np.concatenate([np.ones_like(incl[:, :1]), incl[:, :-1]], axis=1)
    c = np.ones_like(carry) if mutant == 'carry_reset' else carry
    Tb, Ta = c[:, None] * excl, c[:, None] * incl
    return Tb, Ta, np.where(open_, Ta[:, -1], carry)


def _first_sat(valid, Ta, thr, mutant):
    sat = valid & ((Ta < thr) if mutant == 'strict_threshold' else (Ta <= thr))
    return np.where(sat.any(axis=1), sat.argmax(axis=1), Ta.shape[1])


def emulate_fw(sig, rgbs, dl, ts, N, thr, T0=None, G=64, mutant=None):
    """The train forward (and, with T0 and G, the inference walk) on dense (R, K) f32 samples: chunks of G samples, a doubling scan for the
    transmittance with a carry between chunks, lane-wise accumulation and a tree for the ray sums.  Returns total, opacity, depth, rgb (rows),
    ws (R, K) and `stopped`."""
    f = np.float32
    R, K0 = sig.shape
    K = -(-max(K0, 1) // G) * G
    sig, dl, ts, rgbs = _pad(sig.astype(f), K), _pad(dl.astype(f), K), _pad(ts.astype(f), K), _pad(rgbs.astype(f), K)
    N = np.asarray(N, np.int64)
    thr = f(thr)
    lane = np.arange(G)[None, :]
    carry = np.ones(R, f) if T0 is None else T0.astype(f)
    acc = np.zeros((5, R, G), f)
    ws = np.zeros((R, K), f)
    counted, open_, stopped = N.copy(), N > 0, np.zeros(R, bool)
    for c in range(0, K, G):
        if not open_.any():
            break
        sl = slice(c, c + G)
        valid = (c + lane < N[:, None]) & open_[:, None]
        with np.errstate(over='ignore', invalid='ignore'):
            a = np.where(valid, f(1) - _exp32(-(np.where(valid, sig[:, sl], f(0)) * dl[:, sl])), f(0)).astype(f)
        Tb, Ta, carry = _chunk_T(a, carry, open_, mutant)
        fs = _first_sat(valid, Ta, thr, mutant)
        comp = valid & (lane <= fs[:, None])
        if mutant == 'stop_not_composited':
            comp &= lane != fs[:, None]
        w = np.where(comp, a * Tb, f(0)).astype(f)
        for j, coef in enumerate((rgbs[:, sl, 0], rgbs[:, sl, 1], rgbs[:, sl, 2], ts[:, sl])):
            acc[j] += w * np.where(comp, coef, f(0))
        acc[4] += w
        ws[:, sl] = w
        now = open_ & (fs < G)
        counted = np.where(now, c + fs + (1 if mutant == 'count_includes_stop' else 0), counted)
        stopped |= now
        open_ = open_ & ~now & (c + G < N)
    sums = [_tree(acc[j]) for j in range(5)]
    return dict(total=counted, opacity=sums[4], depth=sums[3], rgb=np.stack(sums[:3], axis=1), ws=ws[:, :K0], stopped=stopped)


def emulate_bw(sig, rgbs, dl, ts, N, thr, ws, O, D, RGB, go, gd, gr, gw, mutant=None):
    """The train backward on dense f32 samples: the dL_dws ws sum lane-wise then a tree, the transmittance and the five prefixes as doubling
    scans with carries, suffixes as total - prefix.  go, gd, gw may be None.  Returns dsigma (R, K), drgb (R, K, 3)."""
    f = np.float32
    G = 64
    R, K0 = sig.shape
    K = -(-max(K0, 1) // G) * G
    sig, dl, ts, rgbs, ws = (_pad(np.asarray(v, f), K) for v in (sig, dl, ts, rgbs, ws))
    gw = None if gw is None else _pad(np.asarray(gw, f), K)
    N = np.asarray(N, np.int64)
    thr = f(thr)
    O, D, RGB, gr = np.asarray(O, f), np.asarray(D, f), np.asarray(RGB, f), np.asarray(gr, f)
    go = np.zeros(R, f) if go is None else np.asarray(go, f)
    gd = np.zeros(R, f) if gd is None else np.asarray(gd, f)
    lane = np.arange(G)[None, :]
    part = np.zeros((R, G), f)
    if gw is not None:
        for c in range(0, G if mutant == 'dws_sum_truncated' else K, G):
            valid = c + lane < N[:, None]
            part += np.where(valid, gw[:, c:c + G] * ws[:, c:c + G], f(0))
    dws_sum = _tree(part)
    carry = np.ones(R, f)
    pc = np.zeros((5, R), f)
    ds, dr = np.zeros((R, K), f), np.zeros((R, K, 3), f)
    open_ = N > 0
    for c in range(0, K, G):
        if not open_.any():
            break
        sl = slice(c, c + G)
        valid = (c + lane < N[:, None]) & open_[:, None]
        with np.errstate(over='ignore', invalid='ignore'):
            a = np.where(valid, f(1) - _exp32(-(np.where(valid, sig[:, sl], f(0)) * dl[:, sl])), f(0)).astype(f)
        Tb, Ta, carry = _chunk_T(a, carry, open_, mutant)
        w = (a * Tb).astype(f)
        gwv = np.zeros((R, G), f) if gw is None else np.where(valid, gw[:, sl], f(0))
        coefs = [np.where(valid, v, f(0)) for v in (rgbs[:, sl, 0], rgbs[:, sl, 1], rgbs[:, sl, 2], ts[:, sl])]
        own = [w * v for v in coefs] + [gwv * np.where(valid, ws[:, sl], f(0))]
        pref = []
        for j in range(5):
            incl = pc[j][:, None] + _scan(own[j].astype(f), np.add)
            pc[j] = np.where(open_, incl[:, -1], pc[j])
            pref.append(incl - own[j] if mutant == 'exclusive_prefix' else incl)
        fs = _first_sat(valid, Ta, thr, mutant)
        comp = valid & (lane <= fs[:, None])
        if mutant == 'stop_not_composited':
            comp &= lane != fs[:, None]
        with np.errstate(over='ignore', invalid='ignore'):
            br = (gr[:, 0:1] * (coefs[0] * Ta - (RGB[:, 0:1] - pref[0])) + gr[:, 1:2] * (coefs[1] * Ta - (RGB[:, 1:2] - pref[1])) +
                  gr[:, 2:3] * (coefs[2] * Ta - (RGB[:, 2:3] - pref[2])) + (go * (f(1) - O))[:, None] + gd[:, None] * (coefs[3] * Ta - (D[:, None] - pref[3])) +
                  Ta * gwv - (dws_sum[:, None] - pref[4]))
            ds[:, sl] = np.where(comp, dl[:, sl] * br, f(0))
            dr[:, sl] = np.where(comp[..., None], gr[:, None, :] * w[..., None], f(0))
        open_ = open_ & ~(fs < G) & (c + G < N)
    return ds[:, :K0], dr[:, :K0]


def emulate_distortion_fw(w, dl, t, N, mutant=None):
    """The distortion forward on dense f32 samples: 64-wide prefix scans with carries, lane-wise accumulation and a tree."""
    f = np.float32
    G = 64
    R, K0 = w.shape
    K = -(-max(K0, 1) // G) * G
    w, dl, t = (_pad(np.asarray(v, f), K) for v in (w, dl, t))
    N = np.asarray(N, np.int64)
    lane = np.arange(G)[None, :]
    cw, cwt, acc = np.zeros(R, f), np.zeros(R, f), np.zeros((R, G), f)
    wi_all, wti_all = np.zeros((R, K), f), np.zeros((R, K), f)
    for c in range(0, K, G):
        sl = slice(c, c + G)
        valid = c + lane < N[:, None]
        if not valid.any():
            break
        if mutant == 'distortion_carry_reset':
            cw, cwt = np.zeros(R, f), np.zeros(R, f)
        wv = np.where(valid, w[:, sl], f(0))
        wt = np.where(valid, wv * np.where(valid, t[:, sl], f(0)), f(0))
        wi, wti = cw[:, None] + _scan(wv, np.add), cwt[:, None] + _scan(wt, np.add)
        we = np.concatenate([cw[:, None], wi[:, :-1]], axis=1)
        wte = np.concatenate([cwt[:, None], wti[:, :-1]], axis=1)
        term = f(2) * (wti * we - wi * wte) + f(1) / f(3) * wv * wv * np.where(valid, dl[:, sl], f(0))
        acc += np.where(valid, term, f(0))
        wi_all[:, sl], wti_all[:, sl] = np.where(valid, wi, f(0)), np.where(valid, wti, f(0))
        cw, cwt = wi[:, -1], wti[:, -1]
    return _tree(acc), wi_all[:, :K0], wti_all[:, :K0]


def emulate_distortion_bw(g, wi, wti, w, dl, t, N):
    f = np.float32
    g, wi, wti, w, dl, t = (np.asarray(v, f) for v in (g, wi, wti, w, dl, t))
    R, K = w.shape
    N = np.asarray(N, np.int64)
    mask = np.arange(K)[None, :] < N[:, None]
    last = np.maximum(N - 1, 0)
    rows = np.arange(R)
    ws_sum, wts_sum = wi[rows, last][:, None], wti[rows, last][:, None]
    shift = lambda v: np.concatenate([np.zeros((R, 1), f), v[:, :-1]], axis=1)
    prev = t * shift(wi) - shift(wti)
    v = g[:, None] * f(2) * (prev + (wts_sum - wti - t * (ws_sum - wi)))
    v = v + g[:, None] * f(2) / f(3) * w * dl
    return np.where(mask, v, f(0)).astype(f)


# ------------------------------------------------------------------------------------------------ the cases
def _layout(rng):
    """Lengths (every one of LENGTHS three times and twelve more, weighted to the long ones), the rays laid out in memory with gaps of 1 .. 70
    samples no ray owns, the rows of rays_a a permutation of the memory order, ray_idx a second, different one."""
    extra = rng.choice(LENGTHS, N_RAYS - 3 * len(LENGTHS), p=np.array([1, 1, 1, 1, 1, 1, 2, 2, 2, 4, 6]) / 22)
    lengths = np.concatenate([np.repeat(LENGTHS, 3), extra]).astype(np.int64)
    rng.shuffle(lengths)                                 # memory order
    gaps = rng.integers(1, 71, N_RAYS + 1)
    starts = np.cumsum(gaps[:-1] + np.concatenate([[0], lengths[:-1]]))
    M = int(starts[-1] + lengths[-1] + gaps[-1])
    rows = rng.permutation(N_RAYS)
    while True:
        ray_idx = rng.permutation(N_RAYS)
        if (ray_idx != rows).any() and (ray_idx != np.arange(N_RAYS)).any():
            break
    rays_a = np.stack([ray_idx, starts[rows], lengths[rows]], axis=1).astype(np.int64)
    return rays_a, M


def _samples(rng, rays_a):
    """Per-row dense (R, K_MAX) float32 draws of the `plain` table row."""
    R = rays_a.shape[0]
    sig = rng.uniform(0.0, 4.0, (R, K_MAX)).astype(np.float32)
    dl = rng.uniform(1e-3, 1.1e-2, (R, K_MAX)).astype(np.float32)
    rgbs = rng.random((R, K_MAX, 3)).astype(np.float32)
    ts = (np.float32(0.2) + np.cumsum(dl, axis=1, dtype=np.float64)).astype(np.float32)
    return sig, rgbs, dl, ts


def _assemble(rng, rays_a, M, sig, rgbs, dl, ts, thr, grad_scale=None):
    """Scatter the rows' dense draws into flat arrays (NaN in samples no ray owns) and draw the upstream gradients."""
    idx, mask = dense_index(rays_a, K_MAX)
    R = rays_a.shape[0]
    flat = {}
    for key, v in (('sigmas', sig), ('rgbs', rgbs), ('deltas', dl), ('ts', ts)):
        out = np.full((M,) + v.shape[2:], np.nan, np.float32)
        out[idx[mask]] = v[mask]
        flat[key] = out
    sc = np.ones(R) if grad_scale is None else grad_scale
    by_slot = np.zeros(R)
    by_slot[rays_a[:, 0]] = sc
    gw = np.full(M, 7.0, np.float32)       # finite where nobody reads it
    gw[idx[mask]] = (rng.normal(size=(R, K_MAX)) * sc[:, None]).astype(np.float32)[mask]
    flat.update(rays_a=rays_a, T_threshold=thr, go=(rng.normal(size=R) * by_slot).astype(np.float32), gd=(rng.normal(size=R) * by_slot).astype(np.float32),
                gr=(rng.normal(size=(R, 3)) * by_slot[:, None]).astype(np.float32), gw=gw)
    assert R % 4 != 0
    return _ro(flat)


def plain(seed, thr=1e-4):
    rng = np.random.default_rng(seed)
    rays_a, M = _layout(rng)
    return _assemble(rng, rays_a, M, *_samples(rng, rays_a), thr)


def stops(seed):
    """`plain` with constructed stops (STOP_PLAN): sigma delta = 20 at the chosen sample, the samples before it thinned so that T > 1e-2 there;
    and rays whose density level makes them cross the threshold near a drawn position."""
    rng = np.random.default_rng(seed)
    rays_a, M = _layout(rng)
    sig, rgbs, dl, ts = _samples(rng, rays_a)
    N = rays_a[:, 2]
    used = np.zeros(len(N), bool)
    for length, at in STOP_PLAN:
        row = int(np.nonzero((N == length) & ~used)[0][0])
        used[row] = True
        before = float((sig[row, :at].astype(np.float64) * dl[row, :at]).sum())
        if before > 3.0:
            sig[row, :at] *= np.float32(3.0 / before)
        sig[row, at] = np.float32(20.0) / dl[row, at]
    for row in np.nonzero(~used & (N >= 65))[0][::2]:
        used[row] = True
        at = int(rng.integers(N[row] // 4, N[row] - 1))
        level = 9.5 / float((sig[row, :at + 1].astype(np.float64) * dl[row, :at + 1]).sum())
        sig[row] *= np.float32(level)
    return _assemble(rng, rays_a, M, sig, rgbs, dl, ts, 1e-4)


def tie(seed):
    """T_threshold = 1: a third of the rays open with sigma = 0 (T = 1 <= 1 exactly: they stop at sample 0 having composited w = 0), every other
    ray stops after its first sample.  total_samples is 0 everywhere."""
    rng = np.random.default_rng(seed)
    rays_a, M = _layout(rng)
    sig, rgbs, dl, ts = _samples(rng, rays_a)
    sig[np.nonzero(rays_a[:, 2] > 0)[0][::3], 0] = 0.0
    return _assemble(rng, rays_a, M, sig, rgbs, dl, ts, 1.0)


def extremes(seed):
    """Rays with sigma = 0 throughout, a sample of sigma = 3e38, a sample of sigma = inf (delta > 0), colours of -0.25 and 1.5, upstream
    gradients spanning 1e-6 .. 1e3 per ray.  Returns (case, marks): marks name the rows that were rewritten."""
    rng = np.random.default_rng(seed)
    rays_a, M = _layout(rng)
    sig, rgbs, dl, ts = _samples(rng, rays_a)
    N = rays_a[:, 2]
    has = rng.permutation(np.nonzero(N >= 2)[0])
    marks = dict(zero=has[:5], huge=has[5:10], inf=has[10:15], below=has[15:21], above=has[21:27])
    sig[marks['zero']] = 0.0
    for key, val in (('huge', np.float32(3e38)), ('inf', np.float32(np.inf))):
        for j, row in enumerate(marks[key]):
            at = (0, int(N[row]) - 1, int(N[row]) // 2, min(63, int(N[row]) - 1), min(64, int(N[row]) - 1))[j]
            before = float((sig[row, :at].astype(np.float64) * dl[row, :at]).sum())
            if before > 3.0:
                sig[row, :at] *= np.float32(3.0 / before)
            sig[row, at] = val
    rgbs[marks['below']] = -0.25
    rgbs[marks['above']] = 1.5
    scale = 10.0 ** rng.uniform(-6, 3, len(N))
    scale[:2] = (1e-6, 1e3)
    return _assemble(rng, rays_a, M, sig, rgbs, dl, ts, 1e-4, grad_scale=scale), marks


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case dict (built once, read-only): sigmas, rgbs (M, 3), deltas, ts, gw (M) f32; rays_a (45, 3) i64; go, gd, gr (45[, 3]) f32 per
    SLOT; T_threshold."""
    return {'plain': plain(SEEDS['plain']), 'stops': stops(SEEDS['stops']), 'thr0': plain(SEEDS['thr0'], thr=0.0), 'tie': tie(SEEDS['tie']),
            'extremes': extremes(SEEDS['extremes'])[0]}


CASES = ('plain', 'stops', 'thr0', 'tie', 'extremes')


# ------------------------------------------------------------------------------------------------ judging
def assert_within_budget(got, ref, budget, name, owner=None, rows=None):
    """Every element of `got` within ITS budget of `ref`, none exempt; a non-finite reference or budget is rejected, and so is an error where
    the budget is 0.  owner (per sample: the row of rays_a, -1 for a gap) / rows (per slot: the row) locate the worst element in the message.
    Returns max err / budget."""
    g, r, b = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(budget, np.float64)
    assert g.shape == r.shape == b.shape, f'{name}: shapes {g.shape}, {r.shape}, {b.shape}'
    assert np.isfinite(r).all() and np.isfinite(b).all() and (b >= 0).all(), f'{name}: the reference or the budget is not finite'
    if g.size == 0:
        return 0.0
    err = np.abs(g - r)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / b)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)     # a NaN / inf of `got`, or an error where the budget is 0
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    if not ratio[i] <= 1.0:
        where = f'element {i}'
        if owner is not None:
            where = f'sample {i[0]} (row {int(owner[i[0]])}) {i[1:]}'
        elif rows is not None:
            where = f'slot {i[0]} (row {int(rows[i[0]])}) {i[1:]}'
        raise AssertionError(f'{name}: {where} got {float(g[i])!r} ref {float(r[i])!r} |err| {err[i]:.3e} budget {b[i]:.3e} '
                             f'(err/budget {ratio[i]:.3g}; {int((ratio > 1).sum())} of {ratio.size} over)')
    return float(ratio[i])


def judge_train_fw(got, ref, name):
    """got: total, opacity, depth, rgb per slot and ws (M).  Budgets on every element, total_samples exact, ws exactly 0 outside the support.
    Returns {output: max err / budget}."""
    worst = {k: assert_within_budget(got[k], ref[k], ref['budget'][k], f'{name} {k}', rows=ref['row_of_slot']) for k in ('opacity', 'depth', 'rgb')}
    worst['ws'] = assert_within_budget(got['ws'], ref['ws'], ref['budget']['ws'], f'{name} ws', owner=ref['owner'])
    np.testing.assert_array_equal(np.asarray(got['total'], np.int64), ref['total'], err_msg=f'{name}: total_samples')
    assert (np.asarray(got['ws'])[~ref['support']] == 0).all(), f'{name}: ws is not 0 behind a stop or in a gap'
    return worst


def judge_train_bw(got, ref, name):
    """got: dsigma (M), drgb (M, 3).  Budgets on every element, exactly 0 outside the support."""
    worst = {k: assert_within_budget(got[k], ref[k], ref['budget'][k], f'{name} {k}', owner=ref['owner']) for k in ('dsigma', 'drgb')}
    assert (np.asarray(got['dsigma'])[~ref['support']] == 0).all() and (np.asarray(got['drgb'])[~ref['support']] == 0).all(), \
        f'{name}: a gradient is not 0 behind a stop or in a gap'
    return worst
