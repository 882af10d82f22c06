"""Inputs, a float64 / emulated-f32 numpy model and a per-pixel error budget for the SSIM kernels (nerficg_amd/csrc/ssim.hip) against
oracle/ssim_oracle.c.  Plain module: no test functions.  Used by tests/test_ssim_cases_cpu.py and tests/test_gpu_ssim_edges.py.

The budget
----------
The kernel departs from the oracle only by f32 rounding: of the five blurred moments (mu1, mu2, E[x1^2], E[x2^2], E[x1 x2]) and of the
closing formula.  With u = 2^-24 and |delta| <= u per rounding, a first-order bound of every output is derived per pixel, in float64, from
the inputs alone.

Moments.  One input's path to one output of k_ssim_fwd passes, in each of the two passes, the window constant as f32, the product g * x
(1 rounding) and the rounded additions that follow it; E[x y] carries one more product (g * x * y) in the horizontal pass.  The LDS round
trip between the passes is exact.  Taps are added in ascending order and 0.f + the first product is exact, so tap t sees
TAP_ADDITIONS[t] = 10, 10, 9, ..., 1 additions.  With the constant counted as one rounding against the oracle's double window, the longest
path has
    k = 2 * (1 + 1 + 10) = 24 roundings for mu1, mu2,      k = 24 + 1 = 25 for the three second moments,
and |err(m_q)| <= k u M_q with M_q = the same two-pass blur of |p_q| in float64 (p_q = the exact product).  One k for all taps put the
noise pair above the ceilings below, so the count is kept per tap instead: tap (s, t) of the 11 x 11 window carries
TAP_ROUNDINGS[s] + TAP_ROUNDINGS[t] (+ 1) roundings with TAP_ROUNDINGS = WINDOW_ERROR_U + 1 + TAP_ADDITIONS, and the bound is u times the
blur of |p_q| with those counts as extra weights (`rounded_mass`).  WINDOW_ERROR_U is the actual distance of the kernel's constants from
the double window in units of u (0.16 .. 0.78; two of them are not the nearest f32).  The window's mass sits at the centre taps (6 additions),
so this comes to about 15 u M_q.  A fused multiply-add only removes roundings.  The counts are read off the kernel, not measured.

Closing formula.  Every operation of the kernel's expressions (ssim.hip, k_ssim_fwd: sg1, sg2, sg12, A, B, C, D, iAB, ssim, the three
derivative maps) contributes the propagated error of its operands plus u times its own result; `ssim_budget` writes that out line by line
in the kernel's order.  C1 and C2 reach the kernel and the oracle as the same f32 numbers, so they carry no error.  The f32 divisions are
correctly rounded (hipcc's default; the kernel is not built with fast-math).

Gradient.  k_ssim_bwd forms dL_dmap * map (1 rounding) and blurs it (the same per-tap counts, + 1 for that product), on top of the blur of
|dL_dmap| times the map's own budget, then b0 + 2 img1 b1 + img2 b2 with 2 products and 2 additions.

The oracle itself returns f32: u |value| per output, and its backward pass reads ITS f32 maps (u |map| each, weighted and blurred like the
kernel's).  Both are part of the budget because the comparison is against those f32 numbers.

SAFETY = 1.25 is the one factor on top of the derived bound.  It covers what a first-order bound drops: the second-order terms, of relative
size ~3 e_B / B, which reaches a few percent on flat white where B ~ C2.  Nothing else is added.

Budget maxima on the noise pair, shape (1, 3, 70, 100), seed 174 (`noise_budget_maxima`, SAFETY included):
    map                                          6.73e-05   (asserted below 1e-4)
    gradient, dL_dmap = -1/n (the mean's)        4.88e-04 of max|gradient|   (asserted below 1e-3)
    gradient, dL_dmap ~ N(0, 1)                  1.68e-03 of max|gradient|   (asserted below 2e-3)
The ceilings 1e-4 and 1e-3 are the issue's hand estimates; the computed figures are not far below them, so they stay.  With a random signed
dL_dmap the gradient's scale shrinks (121 signed taps cancel) while a worst-case bound cannot cancel -- it blurs |dL_dmap| -- so that figure
is 3.4 times the constant-upstream one; its ceiling is stated separately instead of loosening the other.  The f32 emulation of
tests/test_ssim_cases_cpu.py sits at 1.4e-06 of the scale there: worst-case counting is ~100 times above the typical error on noise.
For comparison, on flat_white the same budget reaches 1.7e-02 for the map and 28 for dm_dsigma1_sq (|value| ~ 1100): B ~ C2 = 9e-4, and
one ulp of a moment near 1 is ~1e-4 of it.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
SAFETY = 1.25
C1, C2 = 0.01 ** 2, 0.03 ** 2
# SSIM_G of ssim.hip (tests/test_ssim_cases_cpu.py compares it with the source).  Two of the constants are one f32 ulp away from the f32
# nearest to the oracle's double window, so the constant's error is taken per tap from these numbers, in units of u, instead of as 1/2 ulp.
KERNEL_WINDOW = np.array([0.001028380123898387, 0.0075987582094967365, 0.036000773310661316, 0.10936068743467331, 0.21300552785396576,
                          0.26601171493530273, 0.21300552785396576, 0.10936068743467331, 0.036000773310661316, 0.0075987582094967365,
                          0.001028380123898387], np.float32)
# additions after tap t in one pass: taps are added in ascending order and 0.f + the first product is exact
TAP_ADDITIONS = np.array([10, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1], np.float64)
OUTPUTS = ('map', 'dm_dmu1', 'dm_dsigma1_sq', 'dm_dsigma12')
NOISE_MAP_CEILING = 1e-4
NOISE_GRAD_CEILING = 1e-3          # of max|gradient|, dL_dmap = -1/n
NOISE_SIGNED_GRAD_CEILING = 2e-3   # of max|gradient|, dL_dmap ~ N(0, 1): see the module docstring


# ------------------------------------------------------------------------------------------------ image builders: (shape, seed) -> (image, target), f32
def _block(h, w):
    """A block that is never empty, also for one-pixel planes."""
    y0, x0 = h // 4, w // 3
    return slice(y0, y0 + max(1, h // 2)), slice(x0, x0 + max(1, w // 3))


def noise(shape, seed):
    """The pair of tests/test_gpu_ssim_parity.py: uniform noise and the same plus N(0, 0.1), clipped."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape).astype(np.float32)
    b = np.clip(a + 0.1 * rng.normal(size=shape), 0, 1).astype(np.float32)
    return a, b


def _flat(shape, seed, level, sign):
    rng = np.random.default_rng(seed)
    a = np.full(shape, level, np.float32)
    b = np.full(shape, level, np.float32)
    ys, xs = _block(*shape[-2:])
    a[..., ys, xs] = (level + sign * 1e-3 * rng.random(a[..., ys, xs].shape)).astype(np.float32)
    return a, b


def flat_white(shape, seed):
    """Both exactly 1.0, except a block of the image at 1 - 1e-3 * noise."""
    return _flat(shape, seed, 1.0, -1.0)


def flat_black(shape, seed):
    """Both exactly 0.0, except a block of the image at 1e-3 * noise."""
    return _flat(shape, seed, 0.0, 1.0)


def grey_whisper(shape, seed):
    """0.5 plus noise of amplitude 1e-3, drawn independently for both: variance ~3e-7, far below C2."""
    rng = np.random.default_rng(seed)
    a = (0.5 + 1e-3 * (2 * rng.random(shape) - 1)).astype(np.float32)
    b = (0.5 + 1e-3 * (2 * rng.random(shape) - 1)).astype(np.float32)
    return a, b


def silhouette(shape, seed):
    """White background, a dark disc (its level differs per plane); the image's disc is one pixel to the right of the target's."""
    rng = np.random.default_rng(seed)
    h, w = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    level = (0.02 + 0.3 * rng.random(planes)).astype(np.float32).reshape(shape[:-2] + (1, 1))
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx, r = (h - 1) / 2, (w - 1) / 2, max(1.0, min(h, w) / 3)
    disc_b = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    disc_a = (yy - cy) ** 2 + (xx - cx - 1) ** 2 <= r * r
    a = np.where(disc_a, level, np.float32(1.0)).astype(np.float32)
    b = np.where(disc_b, level, np.float32(1.0)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(a, shape)), np.ascontiguousarray(np.broadcast_to(b, shape))


def identical(shape, seed):
    """image == target: the left half flat (a constant per plane), the right half noise.  SSIM is 1, the gradient ~0."""
    rng = np.random.default_rng(seed)
    w = shape[-1]
    a = rng.random(shape).astype(np.float32)
    planes = int(np.prod(shape[:-2]))
    a[..., :, :(w + 1) // 2] = np.linspace(0.0, 1.0, planes, dtype=np.float32).reshape(shape[:-2] + (1, 1))
    return a, a.copy()


def out_of_range(shape, seed):
    """Values in [-0.25, 1.5]: the rasterizer's output is not clamped before the loss."""
    rng = np.random.default_rng(seed)
    a = (-0.25 + 1.75 * rng.random(shape)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.normal(size=shape), -0.25, 1.5).astype(np.float32)
    return a, b


def planes_differ(shape, seed):
    """Every plane has its own mean, its own wave (direction and frequency) and its own noise: no two planes are interchangeable."""
    rng = np.random.default_rng(seed)
    h, w = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.empty((planes, h, w), np.float64)
    for p in range(planes):
        mean = 0.2 + 0.6 * p / max(1, planes - 1)
        ang, freq = 0.7 * p + 0.3, 0.25 + 0.11 * p
        a[p] = mean + 0.15 * np.sin(freq * (np.cos(ang) * xx + np.sin(ang) * yy) + p) + 0.02 * rng.normal(size=(h, w))
    a = np.clip(a, 0, 1).reshape(shape).astype(np.float32)
    b = np.clip(a + 0.05 * rng.normal(size=shape), 0, 1).astype(np.float32)
    return a, b


BUILDERS = {'noise': noise, 'flat_white': flat_white, 'flat_black': flat_black, 'grey_whisper': grey_whisper, 'silhouette': silhouette,
            'identical': identical, 'out_of_range': out_of_range, 'planes_differ': planes_differ}


def case_shape(name):
    """The shape of the content x outputs cases."""
    return (2, 2, 33, 65) if name == 'planes_differ' else (1, 3, 70, 100)


def case_seed(name):
    return 100 + sorted(BUILDERS).index(name)


def upstream(shape, seed):
    """A random signed dL_dmap."""
    return np.random.default_rng(seed + 7919).normal(size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the numpy model (float64, or f32 in the kernel's order)
def gauss_window(sigma=1.5):
    x = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


# roundings on the path of tap t through one pass: the window constant (its actual error against the double window, in u; 0.78 at most),
# the product, the additions after it
WINDOW_ERROR_U = np.abs(KERNEL_WINDOW.astype(np.float64) - gauss_window()) / (gauss_window() * U)
TAP_ROUNDINGS = WINDOW_ERROR_U + 1 + TAP_ADDITIONS


def blur(x, g, dtype=np.float64, y=None, gv=None):
    """Separable 11-tap blur with zero padding over the last two axes, taps added in ascending order into `dtype` accumulators, every
    operation rounded to `dtype` (no FMA).  With `y`, the horizontal pass multiplies g * x * y like the kernel's second moments; `gv` is
    the window of the vertical pass when it differs from the horizontal one."""
    x = np.asarray(x, dtype)
    g = np.asarray(g, dtype)
    gv = g if gv is None else np.asarray(gv, dtype)
    h, w = x.shape[-2:]

    def padded_w(v):
        p = np.zeros(v.shape[:-1] + (w + 10,), dtype)
        p[..., 5:5 + w] = v
        return p
    xp = padded_w(x)
    yp = padded_w(np.asarray(y, dtype)) if y is not None else None
    a = np.zeros(x.shape, dtype)
    for t in range(11):
        term = g[t] * xp[..., t:t + w]
        if yp is not None:
            term = term * yp[..., t:t + w]
        a = a + term
    ap = np.zeros(x.shape[:-2] + (h + 10, w), dtype)
    ap[..., 5:5 + h, :] = a
    b = np.zeros(x.shape, dtype)
    for t in range(11):
        b = b + gv[t] * ap[..., t:t + h, :]
    return b


def model_forward(img1, img2, c1=C1, c2=C2, g=None, dtype=np.float64, variance_bug=False):
    """(map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12) in `dtype`, the expressions in the order of k_ssim_fwd.  c1, c2 enter as the f32 numbers
    the C ABI passes.  `variance_bug`: sigma1^2 formed as E[x1^2] - mu1 mu2 (a mutant for the CPU test)."""
    g = gauss_window() if g is None else g
    t = dtype
    c1, c2 = t(np.float32(c1)), t(np.float32(c2))
    two = t(2)
    mu1, mu2 = blur(img1, g, t), blur(img2, g, t)
    m2, m3, m4 = blur(img1, g, t, img1), blur(img2, g, t, img2), blur(img1, g, t, img2)
    sg1 = m2 - (mu1 * mu2 if variance_bug else mu1 * mu1)
    sg2 = m3 - mu2 * mu2
    sg12 = m4 - mu1 * mu2
    A = mu1 * mu1 + mu2 * mu2 + c1
    B = sg1 + sg2 + c2
    C = two * mu1 * mu2 + c1
    D = two * sg12 + c2
    iAB = t(1) / (A * B)
    ssim = C * D * iAB
    d1 = (mu2 * two * D) * iAB - (mu2 * two * C) * iAB - (mu1 * two * C * D) * iAB / A + (mu1 * two * C * D) * iAB / B
    d2 = (-C * D) * iAB / B
    d3 = (two * C) * iAB
    return ssim, d1, d2, d3


def model_backward(img1, img2, dL_dmap, d1, d2, d3, g=None, dtype=np.float64):
    """dL/dimg1 = G*(dL d1) + 2 img1 G*(dL d2) + img2 G*(dL d3), in the order of k_ssim_bwd."""
    g = gauss_window() if g is None else g
    t = dtype
    dl = np.asarray(dL_dmap, t)
    b = [blur(dl * np.asarray(d, t), g, t) for d in (d1, d2, d3)]
    return b[0] + t(2) * np.asarray(img1, t) * b[1] + np.asarray(img2, t) * b[2]


# ------------------------------------------------------------------------------------------------ the budget
def rounded_mass(p, extra_products):
    """sum over the window of (roundings on the path of tap (s, t)) * g_s g_t |p|: u times this bounds the f32 error of the two-pass blur
    of p to first order.  TAP_ROUNDINGS per pass, plus `extra_products` for the products formed before or inside the horizontal pass."""
    g = gauss_window()
    gc = g * TAP_ROUNDINGS
    ap = np.abs(np.asarray(p, np.float64))
    return blur(ap, gc, gv=g) + blur(ap, g, gv=gc) + extra_products * blur(ap, g)


def ssim_budget(img1, img2, dL_dmap=None, c1=C1, c2=C2):
    """Per-pixel first-order bound (times SAFETY) of |kernel f32 output - oracle f32 output|, float64, from the inputs alone.  Returns a
    dict over OUTPUTS, plus 'grad' when dL_dmap is given.  See the module docstring for the derivation."""
    x1, x2 = np.asarray(img1, np.float64), np.asarray(img2, np.float64)
    g = gauss_window()
    c1, c2 = float(np.float32(c1)), float(np.float32(c2))
    u = U
    mu1, mu2 = blur(x1, g), blur(x2, g)
    m2, m3, m4 = blur(x1 * x1, g), blur(x2 * x2, g), blur(x1 * x2, g)
    e_mu1, e_mu2 = u * rounded_mass(x1, 0), u * rounded_mass(x2, 0)
    e_m2, e_m3, e_m4 = u * rounded_mass(x1 * x1, 1), u * rounded_mass(x2 * x2, 1), u * rounded_mass(x1 * x2, 1)
    a1, a2 = np.abs(mu1), np.abs(mu2)
    sg1, sg2, sg12 = m2 - mu1 * mu1, m3 - mu2 * mu2, m4 - mu1 * mu2
    # sg = m - mu * mu: the product and the difference round once each
    e_sg1 = e_m2 + 2 * a1 * e_mu1 + u * mu1 * mu1 + u * np.abs(sg1)
    e_sg2 = e_m3 + 2 * a2 * e_mu2 + u * mu2 * mu2 + u * np.abs(sg2)
    e_sg12 = e_m4 + a2 * e_mu1 + a1 * e_mu2 + u * a1 * a2 + u * np.abs(sg12)
    A = mu1 * mu1 + mu2 * mu2 + c1
    B = sg1 + sg2 + c2
    C = 2 * mu1 * mu2 + c1
    D = 2 * sg12 + c2
    aC, aD = np.abs(C), np.abs(D)
    # A: two products, two additions, every partial result <= A;  B: two additions;  C: one product (2 * mu1 is exact), one addition;  D: one addition
    e_A = 2 * a1 * e_mu1 + 2 * a2 * e_mu2 + 3 * u * A
    e_B = e_sg1 + e_sg2 + u * np.abs(sg1 + sg2) + u * np.abs(B)
    e_C = 2 * a2 * e_mu1 + 2 * a1 * e_mu2 + 2 * u * a1 * a2 + u * aC
    e_D = 2 * e_sg12 + u * aD
    AB = A * B
    r_iAB = e_A / A + e_B / B + 2 * u           # relative: the product A * B and the division
    e_CD = e_C * aD + aC * e_D
    ssim = C * D / AB
    out = {}
    out['map'] = e_CD / AB + np.abs(ssim) * (r_iAB + 2 * u)          # C * D, (C D) * iAB
    t1, t2 = np.abs(2 * mu2 * D / AB), np.abs(2 * mu2 * C / AB)
    t3, t4 = np.abs(2 * mu1 * C * D / (AB * A)), np.abs(2 * mu1 * C * D / (AB * B))
    e_t1 = (2 * e_mu2 * aD + 2 * a2 * e_D) / AB + t1 * (r_iAB + 2 * u)
    e_t2 = (2 * e_mu2 * aC + 2 * a2 * e_C) / AB + t2 * (r_iAB + 2 * u)
    e_num = 2 * e_mu1 * aC * aD + 2 * a1 * e_CD
    e_t3 = e_num / (AB * A) + t3 * (r_iAB + e_A / A + 4 * u)
    e_t4 = e_num / (AB * B) + t4 * (r_iAB + e_B / B + 4 * u)
    d1 = 2 * mu2 * D / AB - 2 * mu2 * C / AB - 2 * mu1 * C * D / (AB * A) + 2 * mu1 * C * D / (AB * B)
    d2 = -C * D / (AB * B)
    d3 = 2 * C / AB
    out['dm_dmu1'] = e_t1 + e_t2 + e_t3 + e_t4 + 3 * u * (t1 + t2 + t3 + t4)       # three additions of partial sums
    out['dm_dsigma1_sq'] = e_CD / (AB * B) + np.abs(d2) * (r_iAB + e_B / B + 3 * u)  # C * D, * iAB, / B
    out['dm_dsigma12'] = 2 * e_C / AB + np.abs(d3) * (r_iAB + u)                     # (2 C) * iAB
    exact = {'map': ssim, 'dm_dmu1': d1, 'dm_dsigma1_sq': d2, 'dm_dsigma12': d3}
    kernel = dict(out)
    for k in OUTPUTS:
        out[k] = SAFETY * (kernel[k] + u * np.abs(exact[k]))       # + the oracle's own f32 output
    if dL_dmap is not None:
        dl = np.abs(np.asarray(dL_dmap, np.float64))
        E, bb = [], []
        for k in OUTPUTS[1:]:
            ad = np.abs(exact[k])
            # the kernel's map error, its product dl * map and its blur; the oracle's f32 map
            E.append(blur(dl * kernel[k], g) + u * rounded_mass(dl * ad, 1) + u * blur(dl * ad, g))
            bb.append(np.abs(blur(np.asarray(dL_dmap, np.float64) * exact[k], g)))
        w1, w2 = 2 * np.abs(x1), np.abs(x2)
        terms = bb[0] + w1 * bb[1] + w2 * bb[2]
        grad = blur(np.asarray(dL_dmap, np.float64) * d1, g) + 2 * x1 * blur(np.asarray(dL_dmap, np.float64) * d2, g) \
            + x2 * blur(np.asarray(dL_dmap, np.float64) * d3, g)
        # two products and two additions of partial sums <= terms each, then the oracle's f32 output
        out['grad'] = SAFETY * (E[0] + w1 * E[1] + w2 * E[2] + 3 * u * terms + u * np.abs(grad))
        out['grad_terms'] = terms      # |b0| + 2 |img1 b1| + |img2 b2|, for callers that scale dL_dmap on the device
    return out


def assert_within_budget(got, ref, budget, name):
    """Every element of |got - ref| within its budget, none exempt; on failure the worst element is reported.  Returns max err / budget."""
    got, ref, budget = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(budget, np.float64)
    assert got.shape == ref.shape == budget.shape, f'{name}: shapes {got.shape}, {ref.shape}, {budget.shape}'
    assert np.isfinite(ref).all() and np.isfinite(budget).all() and (budget >= 0).all(), f'{name}: reference or budget is not finite'
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / budget)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)          # a NaN / inf of `got`, or an error where the budget is 0
    if ratio.size == 0:
        return 0.0
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    if not ratio[worst] <= 1.0:
        raise AssertionError(f'{name}: element {tuple(int(i) for i in worst)} got {float(got[worst])!r} ref {float(ref[worst])!r} |err| {err[worst]:.3e} '
                             f'budget {budget[worst]:.3e} (err/budget {ratio[worst]:.3g}; {int((ratio > 1).sum())} of {ratio.size} over)')
    return float(ratio[worst])


def noise_budget_maxima():
    """(max of the map's budget, max of the gradient's budget / max|gradient| for dL_dmap = -1/n, the same for a random signed dL_dmap)
    on the noise pair of the content case."""
    shape = case_shape('noise')
    a, b = noise(shape, sum(shape))
    maps = model_forward(a, b)[1:]
    out = []
    for w in (np.full(shape, -1.0 / a.size, np.float32), upstream(shape, sum(shape))):
        bud = ssim_budget(a, b, w)
        out.append(float(bud['grad'].max() / np.abs(model_backward(a, b, w, *maps)).max()))
    return float(bud['map'].max()), out[0], out[1]


# a mistake in the derivation shows as a loose budget here, not as a silent pass elsewhere
NOISE_MAXIMA = noise_budget_maxima()
assert NOISE_MAXIMA[0] < NOISE_MAP_CEILING, NOISE_MAXIMA
assert NOISE_MAXIMA[1] < NOISE_GRAD_CEILING, NOISE_MAXIMA
assert NOISE_MAXIMA[2] < NOISE_SIGNED_GRAD_CEILING, NOISE_MAXIMA
