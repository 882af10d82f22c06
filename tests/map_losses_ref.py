"""Inputs, a float64 numpy restatement and a per-element error budget for the map-loss kernels (nerficg_amd/csrc/map_losses.hip; reference:
src/Optim/Losses/DepthSmoothness.py:31-43, BackgroundEntropy.py:6-8 and depth / (alpha + 1e-6) in front).  Plain module: no test functions.  Used by
tests/test_map_losses_cpu.py, tests/test_gpu_map_losses.py and tests/golden/make_map_losses_golden.py.

The restatement
---------------
`evaluate` computes, in float64, the value, its three terms and the gradients w.r.t. depth, alpha and image, including the `normalize` chain and both
entropy forms.  The constants are the f32 numbers the kernel holds (EPS = f32(1e-6), LO = f32(1e-6), HI = f32(1 - 1e-6)) and the weights are rounded
to f32 first (the C ABI takes floats), so that the comparison measures arithmetic, not constants.  The entropy gradient is zero outside [LO, HI] and
passes at the bounds (torch.clamp); sign(0) = 0.

The inputs
----------
`draw(shape, seed)`: alpha in [0.05, 0.95], normalised depth in [1, 5] (depth = that times alpha, the accumulated depth the rasterizer hands out), image
in [0, 1], all f32.  Kinks (|x| at 0) would make any f32 result differ from f64 by a whole term, so the draw is repeated with the next seed
(seed + 1000, + 2000, ...) until every |lap_x|, |lap_y| -- of depth AND of depth / (alpha + EPS), the tests run both -- and every per-channel |dI| is
>= MARGIN = 1e-3 in float64.  Redrawing the WHOLE array cannot end: a (2, 4, 33, 65) case has ~43 000 such terms, each below the margin with probability
~1e-3 to 2e-3.  So the next seed's draw replaces only the pixels in the centre of an offending term; every test still asserts the margin on all terms
(`margins`), and no element is exempt from the comparison.  `ties()` is the deterministic counterpart: small dyadic numbers, for which f32 arithmetic
is exact and agrees with f64 on every zero -- a constant-depth patch, equal neighbouring image pixels, alpha exactly 0, 1, LO, HI and 0.5.

The budget
----------
First-order propagation of u = 2^-24 through the kernel's own operation sequence; every f32 operation contributes u times its result on top of the
propagated error of its operands (`e_` variables below, absolute errors, float64, computed from the inputs alone).  expf and logf are documented with
1 ulp = 2u; ULP_LIBM = 2 ulps are counted.  -ffp-contract=off: nothing is fused, every operation below rounds.

  forward   s = alpha + EPS                      e_s = u s                       d = depth / s            e_d = 2u |d|        (normalize; else e_d = 0)
            lap = (le + ri) - 2 mi               e_lap = e_d[le] + e_d[ri] + 2 e_d[mi] + u |le + ri| + u |lap|        (2 mi is exact)
            m = sum_c |I_c - I_c'|, mc = m / C   e_mc = (C + 1) u mc             (C differences, C - 1 additions, one division)
            w = expf(-mc)                        e_w = w (e_mc + 2u ULP_LIBM)
            t = |lap w|                          e_t = w e_lap + |lap| e_w + u t
            p = -a logf(a)                       e_p = a 2u ULP_LIBM |log a| + u |p|
            q = (1 - a) logf(1 - a)              e_b = u b, e_q = e_b |log b| + e_b + b 2u ULP_LIBM |log b| + u |q|;   e = p - q: e_e = e_p + e_q + u |e|
            sums: a thread adds 2 terms, 6 shuffle steps, 2 additions across the waves: 9 f32 additions, e_sum = sum e_t + 9u sum t; the double sums,
            the product with 1 / N and the weights are double (2^-53: dropped); the four results are rounded to f32 once: + u |result|.
  backward  gk = g k (k = f32(lambda / N): u; product: u)                     relative 2u;   gk / C: 3u
            c = sign(lap) w gk                   e_c = |c| (e_w / w + 3u)        (the sign is exact while |lap| > e_lap: asserted through MARGIN)
            gd = ((c_x[-1] + c_x[+1]) - 2 c_x[0]) + ((c_y[-1] + c_y[+1]) - 2 c_y[0])
                                                 e_gd = sum of the six e_c (the centre twice) + u (|c_x[-1] + c_x[+1]| + |L_x| + |c_y[-1] + c_y[+1]| + |L_y| + |gd|)
            dL/ddepth = gd / s                   e = e_gd / s + 2u |gd / s|
            dL/dalpha = -(gd d) / s              e = (e_gd |d| + |gd| e_d) / s + 3u |gd d / s|
              + gke t,  t = -(logf(a) + 1)       e_t = 2u ULP_LIBM |log a| + u |t|          (symmetrical: t = logf(1 - a) - logf(a),
                                                 e_t = e_b / b + 2u ULP_LIBM (|log b| + |log a|) + u |t|);  e = |gke| e_t + 3u |gke t|, the sum: + u |dL/dalpha|
            a = |lap| w (gk / C)                 e_a = (gk / C) (w e_lap + |lap| e_w + u |lap| w) + 4u |a|
            dL/dI_c = (a_x[+1] s1 - a_x[0] s0) + (a_y[+1] s3 - a_y[0] s2)     (signs of f32 differences are exact)
                                                 e = the four e_a where the sign is not 0 + u (|g_x| + |g_y| + |dL/dI_c|)
SAFETY = 2 is the one factor on top: it covers the second-order terms and an implementation that orders the same operations differently (torch's f32
evaluation of the reference's own functions -- stored in the fixture -- and of the module's tensor formula, which tests/test_map_losses_cpu.py holds to
this budget on every case before any GPU run: mean() sums pairwise, autograd adds the six terms of dL/dd in another order).  Nothing else is added.

Budget maxima on the named case `NAMED` = shape (2, 4, 33, 65), seed 7, normalize, symmetrical, lambda_smooth 0.1, lambda_entropy 0.01, SAFETY
included (`budget_maxima`; tests/test_map_losses_cpu.py asserts them below the ceilings in brackets):
    loss        1.25e-06 absolute, 3.59e-06 of |loss|          [5e-6 of |loss|]
    dL/ddepth   1.56e-06 of max|gradient|                      [5e-6]
    dL/dalpha   2.05e-06 of max|gradient|                      [5e-6]
    dL/dimage   2.15e-06 of max|gradient|                      [5e-6]
i.e. 25 to 60 u of the tensor's scale: a dozen or two roundings per element, times SAFETY.  The loss figure is dominated by the 9 f32 additions of the
workgroup's sum, counted against the sum of |terms|.  torch's f32 evaluation of the tensor formula uses 0.4 of this budget at the most (the ratios that
tests/test_map_losses_cpu.py prints): worst-case counting against typical rounding, as in tests/ssim_cases.py.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
ULP_LIBM = 2.0
SAFETY = 2.0
MARGIN = 1e-3
EPS = float(np.float32(1e-6))
LO = float(np.float32(1e-6))
HI = float(np.float32(1.0 - 1e-6))
NAMED = dict(shape=(2, 4, 33, 65), seed=7, normalize=True, symmetrical=True, lambda_smooth=0.1, lambda_entropy=0.01)
NAMED_CEILINGS = dict(loss=5e-6, g_depth=5e-6, g_alpha=5e-6, g_image=5e-6)


def f32(v) -> float:
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ the restatement
def _lap(d, axis):
    n = d.shape[axis]
    sl = lambda a, b: tuple(slice(a, b) if k == axis % d.ndim else slice(None) for k in range(d.ndim))
    return d[sl(0, n - 2)] + d[sl(2, n)] - 2.0 * d[sl(1, n - 1)]


def _weights(image, axis):
    """mc = mean_c |I[x] - I[x-1]| at the centres x in [1, n-2] of `axis` (2 = y, 3 = x of (B, C, H, W)), the per-channel differences and w = exp(-mc)."""
    n = image.shape[axis]
    sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(4))
    diff = image[sl(1, n - 1)] - image[sl(0, n - 2)]
    mc = np.abs(diff).mean(axis=1)
    return diff, mc, np.exp(-mc)


def _lap_adjoint(c, axis, n):
    """Scatter of the centre coefficients c (centres 1 .. n-2 along `axis` of a (B, H, W) map) with 1, -2, 1."""
    shape = list(c.shape)
    shape[axis] = n
    out = np.zeros(shape)
    sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(3))
    out[sl(0, n - 2)] += c
    out[sl(2, n)] += c
    out[sl(1, n - 1)] -= 2.0 * c
    return out


def evaluate(depth, alpha, image, lambda_smooth, lambda_entropy, normalize, symmetrical, upstream=1.0):
    """float64 value and gradients.  depth, alpha (B, H, W), image (B, C, H, W).  Returns a dict: loss, S_x, S_y, E, g_depth, g_alpha, g_image."""
    depth, alpha, image = (np.asarray(t, np.float64) for t in (depth, alpha, image))
    ls, le, g = f32(lambda_smooth), f32(lambda_entropy), float(upstream)
    B, H, W = depth.shape
    s = alpha + EPS
    d = depth / s if normalize else depth
    out = dict(S_x=0.0, S_y=0.0, E=0.0, g_depth=np.zeros_like(depth), g_alpha=np.zeros_like(alpha), g_image=np.zeros_like(image))
    if ls != 0.0:
        gd = np.zeros_like(d)
        for axis, key in ((2, 'S_x'), (1, 'S_y')):
            lap = _lap(d, axis)
            diff, mc, w = _weights(image, axis + 1)
            n_terms = lap.size
            out[key] = np.abs(lap * w).mean()
            k = g * ls / n_terms
            gd += _lap_adjoint(np.sign(lap) * w * k, axis, d.shape[axis])
            a = (np.abs(lap) * w * k / image.shape[1])[:, None] * np.sign(diff)          # d term / d I_c[x-1]; minus that at x
            n = image.shape[axis + 1]
            sl = lambda p, q: tuple(slice(p, q) if j == axis + 1 else slice(None) for j in range(4))
            out['g_image'][sl(0, n - 2)] += a
            out['g_image'][sl(1, n - 1)] -= a
        if normalize:
            out['g_depth'] = gd / s
            out['g_alpha'] = -gd * d / s
        else:
            out['g_depth'] = gd
    if le != 0.0:
        a = np.clip(alpha, LO, HI)
        e = -a * np.log(a)
        t = -(np.log(a) + 1.0)
        if symmetrical:
            e = e - (1.0 - a) * np.log(1.0 - a)
            t = np.log(1.0 - a) - np.log(a)
        out['E'] = e.mean()
        out['g_alpha'] = out['g_alpha'] + np.where((alpha >= LO) & (alpha <= HI), g * le / alpha.size * t, 0.0)
    out['loss'] = ls * (out['S_x'] + out['S_y']) + le * out['E']
    return out


# ------------------------------------------------------------------------------------------------ inputs
def margins(depth, alpha, image):
    """The smallest |lap| (of depth and of depth / (alpha + EPS), both directions) and the smallest per-channel |dI|, float64."""
    depth, alpha, image = (np.asarray(t, np.float64) for t in (depth, alpha, image))
    laps = [np.abs(_lap(d, ax)).min() for d in (depth, depth / (alpha + EPS)) for ax in (1, 2)]
    return min(laps), min(np.abs(_weights(image, ax)[0]).min() for ax in (2, 3))


def _raw(shape, seed):
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    alpha = (0.05 + 0.9 * rng.random((B, H, W))).astype(np.float32)
    depth = ((1.0 + 4.0 * rng.random((B, H, W))) * alpha).astype(np.float32)
    image = rng.random((B, C, H, W)).astype(np.float32)
    return depth, alpha, image


def draw(shape, seed=7):
    """(depth, alpha, image), f32, every kink term at least MARGIN from zero (see the module docstring)."""
    depth, alpha, image = _raw(shape, seed)
    B, C, H, W = shape
    for turn in range(1, 200):
        d64, a64, i64 = (t.astype(np.float64) for t in (depth, alpha, image))
        bad_map = np.zeros((B, H, W), bool)
        for d in (d64, d64 / (a64 + EPS)):
            bad_map[:, 1:-1, :] |= np.abs(_lap(d, 1)) < MARGIN
            bad_map[:, :, 1:-1] |= np.abs(_lap(d, 2)) < MARGIN
        bad_img = np.zeros((B, C, H, W), bool)
        bad_img[:, :, 1:-1, :] |= np.abs(_weights(i64, 2)[0]) < MARGIN
        bad_img[:, :, :, 1:-1] |= np.abs(_weights(i64, 3)[0]) < MARGIN
        if not bad_map.any() and not bad_img.any():
            return depth, alpha, image
        nd, na, ni = _raw(shape, seed + 1000 * turn)
        depth = np.where(bad_map, nd, depth)
        alpha = np.where(bad_map, na, alpha)
        image = np.where(bad_img, ni, image)
    raise RuntimeError(f'no kink-free draw for {shape} from seed {seed}')


def ties():
    """Deterministic dyadic inputs, shape (1, 2, 6, 7): depth in multiples of 1/4 with a constant 4 x 4 patch (lap exactly 0 there; use normalize=False),
    image in multiples of 1/16 with runs of equal neighbours, alpha holding exactly 0, 1, LO, HI and 0.5."""
    yy, xx = np.mgrid[0:6, 0:7]
    depth = (((3 * yy * yy + 5 * xx * xx + 7 * yy * xx) % 11) * 0.25 + 1.0).astype(np.float32)
    depth[1:5, 1:5] = 2.5
    image = np.stack([((yy * 3 + xx * 5) % 8) / 16.0, ((yy + 2 * xx) % 5) / 16.0]).astype(np.float32)
    image[:, 2:4, 2:5] = 0.25                                         # equal neighbours in both directions, both channels
    alpha = (0.125 + ((yy * 7 + xx * 3) % 13) / 16.0).astype(np.float32)
    alpha[0, 0], alpha[0, 1], alpha[0, 2], alpha[0, 3], alpha[0, 4] = 0.0, 1.0, np.float32(LO), np.float32(HI), 0.5
    alpha[5, 6], alpha[5, 5] = np.nextafter(np.float32(LO), np.float32(0)), np.nextafter(np.float32(HI), np.float32(2))   # one ulp outside either bound
    return depth[None], alpha[None], image[None]


# ------------------------------------------------------------------------------------------------ the budget
def _shift(a, axis, k):
    """a[x + k] along axis, zero where that leaves the array."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    src = tuple(slice(max(k, 0), n + min(k, 0)) if j == axis else slice(None) for j in range(a.ndim))
    dst = tuple(slice(max(-k, 0), n + min(-k, 0)) if j == axis else slice(None) for j in range(a.ndim))
    out[dst] = a[src]
    return out


def _pad_centres(c, axis, n):
    """Centre values (1 .. n-2 along axis) -> full map, zero at the two ends."""
    shape = list(c.shape)
    shape[axis] = n
    out = np.zeros(shape)
    out[tuple(slice(1, n - 1) if j == axis else slice(None) for j in range(c.ndim))] = c
    return out


def budget(depth, alpha, image, lambda_smooth, lambda_entropy, normalize, symmetrical, upstream=1.0):
    """Absolute error budgets (SAFETY included) for what `evaluate` returns: a float for loss, S_x, S_y, E and an array per gradient.  The derivation is the
    module docstring's, line by line."""
    depth, alpha, image = (np.asarray(t, np.float64) for t in (depth, alpha, image))
    ls, le, g = f32(lambda_smooth), f32(lambda_entropy), abs(float(upstream))
    B, H, W = depth.shape
    C = image.shape[1]
    u = U
    s = alpha + EPS
    d = depth / s if normalize else depth
    e_d = 2 * u * np.abs(d) if normalize else np.zeros_like(d)
    bud = dict(S_x=0.0, S_y=0.0, E=0.0, g_depth=np.zeros_like(depth), g_alpha=np.zeros_like(alpha), g_image=np.zeros_like(image))
    e_loss = 0.0
    if ls != 0.0:
        e_gd = np.zeros_like(d)
        gd = np.zeros_like(d)
        round_gd = np.zeros_like(d)
        g_img_parts = []
        for axis, key in ((2, 'S_x'), (1, 'S_y')):
            n = d.shape[axis]
            sl = lambda p, q: tuple(slice(p, q) if j == axis else slice(None) for j in range(3))
            le_, ri, mi = d[sl(0, n - 2)], d[sl(2, n)], d[sl(1, n - 1)]
            lap = le_ + ri - 2 * mi
            e_lap = e_d[sl(0, n - 2)] + e_d[sl(2, n)] + 2 * e_d[sl(1, n - 1)] + u * np.abs(le_ + ri) + u * np.abs(lap)
            diff, mc, w = _weights(image, axis + 1)
            e_w = w * ((C + 1) * u * mc + 2 * u * ULP_LIBM)
            t = np.abs(lap * w)
            e_t = w * e_lap + np.abs(lap) * e_w + u * t
            N = t.size
            bud[key] = ((e_t.sum() + 9 * u * t.sum()) / N + u * t.mean())
            e_loss += ls * (e_t.sum() + 9 * u * t.sum()) / N
            gk = g * ls / N
            c = _pad_centres(np.sign(lap) * w * gk, axis, n)
            e_c = _pad_centres(w * gk * (e_w / w + 3 * u), axis, n)
            pair = _shift(c, axis, -1) + _shift(c, axis, 1)
            L = pair - 2 * c
            gd += L
            e_gd += _shift(e_c, axis, -1) + _shift(e_c, axis, 1) + 2 * e_c
            round_gd += u * (np.abs(pair) + np.abs(L))
            a = _pad_centres(np.abs(lap) * w * gk / C, axis, n)
            e_a = _pad_centres((gk / C) * (w * e_lap + np.abs(lap) * e_w + u * np.abs(lap) * w), axis, n) + 4 * u * a
            sgn0 = np.sign(image - _shift(image, axis + 1, -1))          # sign(I[x] - I[x-1]), the term centred at x
            sgn1 = np.sign(_shift(image, axis + 1, 1) - image)           # sign(I[x+1] - I[x]), the term centred at x + 1
            a1, e_a1 = _shift(a, axis, 1), _shift(e_a, axis, 1)
            part = a1[:, None] * sgn1 - a[:, None] * sgn0
            g_img_parts.append(part)
            bud['g_image'] += e_a1[:, None] * np.abs(sgn1) + e_a[:, None] * np.abs(sgn0) + u * np.abs(part)
        bud['g_image'] += u * np.abs(g_img_parts[0] + g_img_parts[1])
        e_gd += round_gd + u * np.abs(gd)
        if normalize:
            bud['g_depth'] = e_gd / s + 2 * u * np.abs(gd / s)
            bud['g_alpha'] = (e_gd * np.abs(d) + np.abs(gd) * e_d) / s + 3 * u * np.abs(gd * d / s)
            ga_n = -gd * d / s
        else:
            bud['g_depth'] = e_gd
            ga_n = np.zeros_like(d)
    else:
        ga_n = np.zeros_like(d)
    if le != 0.0:
        a = np.clip(alpha, LO, HI)
        la = np.log(a)
        p = -a * la
        e_e = a * 2 * u * ULP_LIBM * np.abs(la) + u * np.abs(p)
        e_t = 2 * u * ULP_LIBM * np.abs(la) + u * np.abs(la + 1.0)
        tt = -(la + 1.0)
        if symmetrical:
            b = 1.0 - a
            lb = np.log(b)
            e_b = u * b
            q = b * lb
            e_e = e_e + e_b * np.abs(lb) + e_b + b * 2 * u * ULP_LIBM * np.abs(lb) + u * np.abs(q) + u * np.abs(p - q)
            tt = lb - la
            e_t = e_b / b + 2 * u * ULP_LIBM * (np.abs(lb) + np.abs(la)) + u * np.abs(tt)
            p = p - q
        N = alpha.size
        bud['E'] = (e_e.sum() + 9 * u * np.abs(p).sum()) / N + u * abs(p.mean())
        e_loss += le * (e_e.sum() + 9 * u * np.abs(p).sum()) / N
        gke = g * le / N
        inside = (alpha >= LO) & (alpha <= HI)
        term = np.where(inside, gke * tt, 0.0)
        bud['g_alpha'] = bud['g_alpha'] + np.where(inside, gke * e_t + 3 * u * np.abs(term), 0.0) + u * np.abs(ga_n + term)
    val = evaluate(depth, alpha, image, lambda_smooth, lambda_entropy, normalize, symmetrical, upstream)
    bud['loss'] = e_loss + u * abs(val['loss'])
    return {k: SAFETY * v for k, v in bud.items()}


def budget_maxima(case=NAMED):
    """The budget's size on one named case, as (absolute loss budget, loss budget / |loss|, max budget / max|gradient| per gradient)."""
    depth, alpha, image = draw(case['shape'], case['seed'])
    args = (depth, alpha, image, case['lambda_smooth'], case['lambda_entropy'], case['normalize'], case['symmetrical'])
    val, bud = evaluate(*args), budget(*args)
    out = dict(loss_abs=bud['loss'], loss=bud['loss'] / abs(val['loss']))
    for k in ('g_depth', 'g_alpha', 'g_image'):
        out[k] = float(bud[k].max() / np.abs(val[k]).max())
    return out


def assert_within_budget(got, want, bud, what):
    """Every element: |got - want| <= budget.  Returns the largest error / budget ratio."""
    got, want, bud = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bud, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    exact = err == 0
    ratio = np.where(exact, 0.0, err / np.where(bud > 0, bud, np.finfo(np.float64).tiny))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f'{what}: {int((ratio > 1).sum())} of {ratio.size} elements over budget, worst ratio {worst:.3f} (error {float(err.flat[ratio.argmax()]):.3e})'
    return worst


# ------------------------------------------------------------------------------------------------ the cases
# the smallest shapes at which the kernels can go wrong (32 x 16 tiles, 64-lane waves): one term per direction; one direction degenerate; odd sizes around a
# tile edge; two images, two tiles each way, both ends of the channel count; and more than 4096 workgroups (one trip of k_map_reduce takes 4 x 1024 partials)
SHAPES = ((1, 3, 3, 3), (1, 3, 3, 40), (1, 3, 40, 3), (1, 1, 17, 33), (2, 4, 33, 65))
MANY_WORKGROUPS = (2, 1, 529, 2081)          # 2 * ceil(529 / 16) * ceil(2081 / 32) = 4488 workgroups
LAMBDA_SMOOTH, LAMBDA_ENTROPY = 0.1, 0.01
GOLDEN_CONFIGS = ((True, False), (False, True))          # (normalize, symmetrical) of the stored float64 results


def golden_key(shape, normalize, symmetrical):
    return 'x'.join(map(str, shape)) + f'_n{int(normalize)}_s{int(symmetrical)}'
WEIGHTS = ((LAMBDA_SMOOTH, 0.0), (0.0, LAMBDA_ENTROPY), (LAMBDA_SMOOTH, LAMBDA_ENTROPY))          # each weight alone, then both
CONFIGS = tuple((n, s, w) for n in (False, True) for s in (False, True) for w in WEIGHTS)
MANY_CONFIGS = ((True, True, WEIGHTS[2]), (False, False, WEIGHTS[2]))
TIES_CONFIGS = tuple((False, s, w) for s in (False, True) for w in WEIGHTS)                     # normalize=False: the patch's zeros are exact
UPSTREAM = 0.625                                                                                # exact in f32; the torch-f32 check uses 1 (loss.backward())


def all_cases():
    """(name, shape or 'ties', normalize, symmetrical, (lambda_smooth, lambda_entropy)) of every comparison the CPU and the GPU test make."""
    out = [(s, c) for s in SHAPES for c in CONFIGS] + [(MANY_WORKGROUPS, c) for c in MANY_CONFIGS] + [('ties', c) for c in TIES_CONFIGS]
    return [(('x'.join(map(str, s)) if s != 'ties' else s) + f'-n{int(n)}-s{int(sy)}-ls{w[0]}-le{w[1]}', s, n, sy, w) for s, (n, sy, w) in out]


import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def inputs(shape):
    return ties() if shape == 'ties' else draw(shape)


@functools.lru_cache(maxsize=64)
def reference(shape, normalize, symmetrical, weights, upstream=1.0):
    """(value dict, budget dict) of one case, computed once and shared; callers leave the arrays alone."""
    depth, alpha, image = inputs(shape)
    args = (depth, alpha, image, weights[0], weights[1], normalize, symmetrical, upstream)
    return evaluate(*args), budget(*args)
