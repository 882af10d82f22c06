"""A float64 statement of one inference frame's compositing, a per-pixel f32 error budget for it, an f32 emulation and synthetic tiled frames.
Plain module: no test functions.  Used by tests/test_image_composite_ref_cpu.py and tests/test_gpu_image_composite.py.

What is stated
--------------
The last stage of the fused InstantNGP frame (include/nerficg_hip.h, group 6, step 4) in the reference's semantics:
  * raymarching.cu:11-13 and :370 -- the step of a sample is re-derived from its position, dt = clamp(t * esf, sqrt3 / max_samples,
    sqrt3 * 2 * cascades / grid_size): the inference march passes `cascades` where calc_dt expects `scale`;
  * volumerendering.cu:205-249 -- front to back, a = 1 - exp(-sigma dt), w = a T, sums of w c, w t, w, T <- T (1 - a); the ray composites the
    sample that brings T <= T_threshold and then stops;
  * Renderer.py:133-138 -- alpha clamped to [0, 1], the background blended with 1 - alpha, rgb clamped, depth = depth / alpha where
    1 - alpha < 1 and 0 elsewhere;
  * sigma = exp(h0) (TruncExp), h0 the fp16 network output widened.
Inputs are the tiled layout: `packed` fp16 (h0, r, g, b) at slot (tile_off[lt] + k) * 64 + lane, `ts` compact (same slot) or the count pass's
arena (((lt * arena_rows + k) << 6) + lane), ray_cnt[lt * 64 + lane], lane = (y & 7) * 8 + (x & 7) of an 8 x 8 pixel tile, a shard = the
tiles [tile_begin, tile_begin + n_tiles) of the row-major tile grid.  row_capacity > 0: sample k of a tile exists only if
tile_off[lt] + k < row_capacity.  The f32 arguments of the C ABI (esf, T_threshold, the background) enter as the f32 numbers they are.

The budget (`composite_image_budget`)
-------------------------------------
The compositing is a short serial f32 recurrence on known inputs, so every output gets a first-order bound of its f32 rounding error, in
float64, from the inputs alone.  u = 2^-24, |delta| <= u |result| per rounding.  Per sample, with x = sigma dt, e = exp(-x), a = 1 - e:
    dt       the clamp of t * esf (1 rounding) or a clamp constant (sqrt3 / max_samples: 1 rounding; sqrt3 * 2 * cascades / grid: 2) -> 2 u dt
    sigma    expf(h0): EXPF_ULPS ulp = 2 EXPF_ULPS u relative (h0 is exact)
    x        the product: u                                      -> x carries (2 + 2 EXPF_ULPS + 1) u relative
    e        the fast exponential = exp2(x * log2 e): the argument's error moves e by e |x| (rel_x + 2 u) (the rounded product and log2 e
             held as f32: |x| u each), the exp2 unit adds EXP2_ULPS ulp OF e (an ulp of a number in [1/2, 1) is u, not 2 u: that halves
             the budget of thin samples, whose whole error is this ulp).  x = 0 exactly (sigma = 0): e = 1 exactly, no error at all.
    a        1 - e: exact for e >= 1/2 (Sterbenz), else u a
    1 - a    exact: for e >= 1/2 it is e again, else a >= 1/2 and Sterbenz applies once more -> 1 - a carries a's error, no new rounding
    w        a T: e_w = e_a T + a e_T + u w
    colours  one FMA per channel: e_r += e_w |c| + u |r'|      (c is exact fp16)
    depth    product and sum: e_d += e_w |t| + u w |t| + u |d'|
    opacity  sum: e_o += e_w + u o'
    T        T (1 - a): e_T' = e_T (1 - a) + T e_a + u T'
Finalisation: the clamps are 1-Lipschitz (no error of their own); Tr = 1 - alpha rounds once (u Tr); fma(Tr, bg, r) rounds once; the division
rounds once.  rgb = r + (1 - o) bg sees the SAME w_k in r and in o, so sample k moves it by e_w |c_k - bg| and not by e_w (|c_k| + |bg|): the
sum is kept with that coefficient and used where the opacity clamp cannot act (o + e_o < 1); elsewhere e_r + e_o |bg|.  The roundings of the
opacity additions reach rgb times |bg|.  depth = d / alpha: (e_d + depth e_alpha) / (alpha - e_alpha) + u depth while alpha > 2 e_alpha.  Below
that the quotient is not determined by the inputs at f32 precision -- the f32 pixel may even take the no-hit branch, alpha = 0 -> depth 0 --
and all that holds is that a weighted mean of the ray's positions lies among them: the budget is max|t| + |depth| there.
SAFETY = 1.25 covers the second-order terms.  Nothing else is added.

EXPF_ULPS = 1 and EXP2_ULPS = 1: NOT MEASURED.  Neither the ROCm device-library documentation nor an accuracy figure of the exp2 unit is part of
this repository's documents or of the programming guides at hand, so both are taken as 1 ulp, the figure OpenCL-style device libraries state
for expf and the coarsest a hardware transcendental is usually specified to.  They are not tuned against any kernel output.

Threshold rays.  The early-out is a discontinuity: a ray whose T after a sample (not its last) lies within its own budget of T_threshold may
stop one sample earlier or later in f32.  Such a ray is reported (`threshold`) and its bounds are widened by everything the rest of the ray can
add: at most T_k for alpha, T_k max|c| (max|c - bg|) for rgb, T_k max|t| for the depth sum, through the finalisation.  A comparison that is
exact (e_T = 0, e.g. T = 1 after a sample with sigma = 0 against T_threshold = 1) is no threshold ray.  A ray with a sample whose t * esf lies
within one rounding of a clamp constant is reported too (the f32 clamp may pick the other branch); the clamp is continuous, so nothing needs
widening.  Every case below keeps threshold rays at or below 1 % of the rays that have samples (asserted on the CPU).

Budget maxima per case (SAFETY included; tests/test_image_composite_ref_cpu.py prints them) and how far the f32 emulation (`composite_image_f32`,
the same operation order in np.float32 with np.exp for both exponentials) stays below: see that module's docstring.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
SAFETY = 1.25
EXPF_ULPS = 1.0     # expf: not measured, see the module docstring
EXP2_ULPS = 1.0     # the exp2 unit behind the fast exponential: not measured
SQRT3 = float(np.float32(1.73205080757))      # raymarching.cu:4
TILE_W = TILE_H = 8
COUNTS = (0, 1, 2, 7, 8, 9, 16, 17, 40, 70)
THRESHOLD_RAY_CAP = 0.01
PLAIN_CEILING = 1e-5    # alpha and rgb budget maxima on `plain`


def step_constants(cascades, grid_size, max_samples):
    """(dt_min, dt_max) of raymarching.cu:11-13 as :370 calls it -- `cascades` in the upper clamp."""
    return SQRT3 / max_samples, SQRT3 * 2 * cascades / grid_size


def ulp_f32(v):
    """The spacing of f32 at |v| (normal range)."""
    v = np.abs(np.asarray(v, np.float64))
    with np.errstate(divide='ignore'):
        ex = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** (np.maximum(ex, -126.0) - 23), 0.0)


# ------------------------------------------------------------------------------------------------ layout
def _geometry(width, height, tile_begin, n_tiles):
    """Per ray slot q = lt * 64 + lane of the shard: pixel index (or -1 outside the image)."""
    tiles_x = (width + TILE_W - 1) // TILE_W
    lt = np.repeat(np.arange(n_tiles, dtype=np.int64), 64)
    lane = np.tile(np.arange(64, dtype=np.int64), n_tiles)
    tile = tile_begin + lt
    px = (tile % tiles_x) * TILE_W + (lane & 7)
    py = (tile // tiles_x) * TILE_H + (lane >> 3)
    inside = (px < width) & (py < height)
    return lt, lane, np.where(inside, py * width + px, -1)


def _walk(packed, ts, ray_cnt, tile_off, width, height, tile_begin, n_tiles, cascades, esf, grid_size, max_samples, T_threshold, bg3,
          row_capacity=0, arena_rows=0):
    """The reference and its budget in one front-to-back pass, vectorised over the shard's rays."""
    packed = np.asarray(packed).reshape(-1, 4)
    assert packed.dtype == np.float16
    ts = np.asarray(ts, np.float32).reshape(-1)
    ray_cnt = np.asarray(ray_cnt).reshape(-1).astype(np.int64)
    tile_off = np.asarray(tile_off).reshape(-1).astype(np.int64)
    lt, lane, pix = _geometry(width, height, tile_begin, n_tiles)
    inside = pix >= 0
    row0 = tile_off[lt]
    cap = np.int64(row_capacity) if row_capacity > 0 else np.iinfo(np.int64).max
    N = np.where(inside, np.minimum(ray_cnt[:n_tiles * 64], np.maximum(cap - row0, 0)), 0)
    esf = float(np.float32(esf))
    thr = float(np.float32(T_threshold))
    bg = np.asarray(bg3, np.float32).astype(np.float64).reshape(3)
    dt_min, dt_max = step_constants(cascades, grid_size, max_samples)
    u = U
    R = n_tiles * 64
    z = lambda *s: np.zeros((R,) + s)
    T, r, d, o = np.ones(R), z(3), z(), z()
    e_T, e_rc, e_rb, e_rr, e_d, e_ow, e_oo = z(), z(3), z(3), z(3), z(), z(), z()
    alive = N > 0
    stop = np.full(R, -1, np.int64)
    thr_ray, widen = np.zeros(R, bool), z()
    max_c, max_cb, max_t = z(), z(), z()
    regimes = np.zeros(3, np.int64)        # composited samples on the lower clamp, on t * esf, on the upper clamp
    at8 = np.zeros((R, 2), bool)           # (stopped before sample 8, composites sample 8)
    for k in range(int(N.max(initial=0))):
        has = k < N
        slot = np.where(has, (row0 + k) * 64 + lane, 0)
        tslot = np.where(has, ((lt * arena_rows + k) << 6) + lane, 0) if arena_rows > 0 else slot
        v = packed[slot].astype(np.float64)
        h0, c, t = v[:, 0], v[:, 1:], ts[tslot].astype(np.float64)
        # what the rest of a ray could still add, whether or not the reference goes there
        max_c = np.where(has, np.maximum(max_c, np.abs(c).max(axis=1)), max_c)
        max_cb = np.where(has, np.maximum(max_cb, np.abs(c - bg).max(axis=1)), max_cb)
        max_t = np.where(has, np.maximum(max_t, np.abs(t)), max_t)
        act = alive & has
        if k == 8:
            at8[:, 0], at8[:, 1] = ~alive & (N > 8), act
        if not act.any():
            continue
        te = t * esf
        dt = np.maximum(dt_min, np.minimum(te, dt_max))
        if esf > 0:
            near = (np.abs(te - dt_min) <= u * np.abs(te)) | (np.abs(te - dt_max) <= u * np.abs(te))
            thr_ray |= act & near
        regimes += np.array([(act & (te <= dt_min)).sum(), (act & (te > dt_min) & (te < dt_max)).sum(), (act & (te >= dt_max)).sum()])
        with np.errstate(over='ignore', invalid='ignore'):
            sigma = np.exp(np.where(act, h0, 0.0))
            x = sigma * dt
            e = np.exp(-x)
            a = -np.expm1(-x)
            rel_x = (2 + 2 * EXPF_ULPS + 1) * u
            e_e = np.where(x == 0, 0.0, e * x * (rel_x + 2 * u) + EXP2_ULPS * ulp_f32(e))
            e_a = e_e + np.where(e >= 0.5, 0.0, u * a)
            w = a * T
            e_w = e_a * T + a * e_T + u * w
            r_new = r + w[:, None] * c
            d_new = d + w * t
            o_new = o + w
            T_new = T * e
            e_Tn = e_T * e + T * e_a + np.where(e == 1.0, 0.0, u * T_new)     # a product with exactly 1 does not round
        m = act
        m3 = m[:, None]
        e_rc = np.where(m3, e_rc + e_w[:, None] * np.abs(c), e_rc)
        e_rb = np.where(m3, e_rb + e_w[:, None] * np.abs(c - bg), e_rb)
        e_rr = np.where(m3, e_rr + u * np.abs(r_new), e_rr)
        e_d = np.where(m, e_d + e_w * np.abs(t) + u * w * np.abs(t) + u * np.abs(d_new), e_d)
        e_ow = np.where(m, e_ow + e_w, e_ow)
        e_oo = np.where(m, e_oo + u * o_new, e_oo)
        r, d, o = np.where(m3, r_new, r), np.where(m, d_new, d), np.where(m, o_new, o)
        T, e_T = np.where(m, T_new, T), np.where(m, e_Tn, e_T)
        last = k + 1 >= N
        stops = T <= thr
        ambiguous = m & ~last & ((T - SAFETY * e_T <= thr) != (T + SAFETY * e_T <= thr))
        widen = np.where(ambiguous & (widen == 0), T, widen)      # the first ambiguous early-out of a ray has the largest T
        done = m & (stops | last)
        stop = np.where(done, k, stop)
        alive = alive & ~done
    thr_ray |= widen > 0
    return dict(lt=lt, lane=lane, pix=pix, inside=inside, N=N, T=T, r=r, d=d, o=o, e_T=e_T, e_rc=e_rc, e_rb=e_rb, e_rr=e_rr, e_d=e_d, e_ow=e_ow,
                e_oo=e_oo, stop=stop, threshold=thr_ray, widen=widen, max_c=max_c, max_cb=max_cb, max_t=max_t, bg=bg, regimes=regimes, at8=at8)


def _finish(s):
    """Renderer.py:133-138 on the walk's sums, and the budget through it.  Rows = the shard's ray slots."""
    u, bg = U, s['bg']
    o, r, d = s['o'], s['r'], s['d']
    al = np.clip(o, 0.0, 1.0)
    Tr = 1.0 - al
    val = r + Tr[:, None] * bg
    rgb = np.clip(val, 0.0, 1.0)
    hit = Tr < 1.0
    depth = np.where(hit, d / np.where(al > 0, al, 1.0), 0.0)
    W = s['widen']
    e_o = s['e_ow'] + s['e_oo']
    e_al = e_o + W
    free = (o + SAFETY * e_al < 1.0)[:, None]       # the opacity clamp cannot act: r and (1 - o) bg move together
    lin = np.where(free, s['e_rb'] + W[:, None] * s['max_cb'][:, None], s['e_rc'] + (s['e_ow'] + W)[:, None] * np.abs(bg) + W[:, None] * s['max_c'][:, None])
    e_rgb = lin + s['e_rr'] + (s['e_oo'] + u * Tr)[:, None] * np.abs(bg) + u * np.abs(val)
    e_dsum = s['e_d'] + W * s['max_t']
    firm = al > 2 * SAFETY * e_al
    with np.errstate(divide='ignore', invalid='ignore'):
        e_depth = np.where(firm, (e_dsum + np.abs(depth) * e_al) / (al - SAFETY * e_al) + u * np.abs(depth), s['max_t'] + np.abs(depth))
    e_depth = np.where(s['N'] > 0, e_depth, 0.0)     # a ray without samples: depth is 0, exactly
    return (rgb, al, depth), (SAFETY * e_rgb, SAFETY * e_al, np.where(firm, SAFETY, 1.0) * e_depth)


def composite_image_f64(packed, ts, ray_cnt, tile_off, width, height, tile_begin, n_tiles, cascades, esf, grid_size, max_samples, T_threshold, bg3,
                        row_capacity=0, arena_rows=0, with_budget=False):
    """float64 reference of one shard.  Returns a dict: 'pix' (pixel index of every ray of the shard that lies inside the image, in slot
    order), 'rgb' (n, 3), 'alpha' (n), 'depth' (n) for those pixels, and per ray SLOT (n_tiles * 64 entries) 'stop' = index of the sample at which the ray
    stopped (-1: no sample), 'n' = samples the ray has, 'inside'.  with_budget: also 'budget' = {'rgb', 'alpha', 'depth'} per pixel,
    'threshold' (per slot: a threshold ray), 'regimes' (composited samples on the lower clamp / on t * esf / on the upper clamp), 'T' / 'e_T' (per slot: the final transmittance and its budget),
    'at8' (per slot: stopped before sample 8, composites sample 8)."""
    s = _walk(packed, ts, ray_cnt, tile_off, width, height, tile_begin, n_tiles, cascades, esf, grid_size, max_samples, T_threshold, bg3,
              row_capacity, arena_rows)
    (rgb, al, depth), (b_rgb, b_al, b_depth) = _finish(s)
    q = s['inside']
    out = dict(pix=s['pix'][q], rgb=rgb[q], alpha=al[q], depth=depth[q], stop=s['stop'], n=s['N'], inside=q)
    if with_budget:
        out.update(T=s['T'], e_T=SAFETY * s['e_T'], budget=dict(rgb=b_rgb[q], alpha=b_al[q], depth=b_depth[q]), threshold=s['threshold'], regimes=s['regimes'], at8=s['at8'])
    return out


def composite_image_budget(*args, **kw):
    """Per-pixel first-order f32 error bound (times SAFETY) of rgb, alpha and depth, from the inputs alone (module docstring).  Same arguments
    as composite_image_f64.  Returns ({'rgb', 'alpha', 'depth'}, threshold) -- threshold per ray slot."""
    out = composite_image_f64(*args, with_budget=True, **kw)
    return out['budget'], out['threshold']


# ------------------------------------------------------------------------------------------------ the same operation order in np.float32
def composite_image_f32(packed, ts, ray_cnt, tile_off, width, height, tile_begin, n_tiles, cascades, esf, grid_size, max_samples, T_threshold, bg3,
                        row_capacity=0, arena_rows=0, mutant=None):
    """An emulation in np.float32: every operation rounded where an f32 compositor rounds it (the colour sums and the background blend as
    fused multiply-adds, the depth and opacity sums as product + sum), np.exp for both exponentials.  Same return as composite_image_f64
    (no budget).  `mutant`: one wrong variant, for the tests that show the comparison has teeth:
    'strict_threshold' (T < thr), 'depth_dt' (depth sums w dt), 'no_dt_max', 'skip_last', 'scale_clamp' (scale = 2^(cascades - 2) in the upper clamp)."""
    f = np.float32
    packed = np.asarray(packed).reshape(-1, 4)
    ts = np.asarray(ts, f).reshape(-1)
    ray_cnt = np.asarray(ray_cnt).reshape(-1).astype(np.int64)
    tile_off = np.asarray(tile_off).reshape(-1).astype(np.int64)
    lt, lane, pix = _geometry(width, height, tile_begin, n_tiles)
    inside = pix >= 0
    row0 = tile_off[lt]
    cap = np.int64(row_capacity) if row_capacity > 0 else np.iinfo(np.int64).max
    N = np.where(inside, np.minimum(ray_cnt[:n_tiles * 64], np.maximum(cap - row0, 0)), 0)
    esf, thr = f(esf), f(T_threshold)
    bg = np.asarray(bg3, f).reshape(3)
    clamp_scale = f(cascades) if mutant != 'scale_clamp' else f(2.0 ** (cascades - 2))
    dt_min, dt_max = f(SQRT3) / f(max_samples), f(SQRT3) * f(2) * clamp_scale / f(grid_size)
    if mutant == 'no_dt_max':
        dt_max = f(np.inf)
    R = n_tiles * 64
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    # np.exp of the f32 argument, evaluated in double and rounded once: numpy's vectorised f32 exp is specified to ~2.5 ulp, outside the 1 ulp
    # the budget grants the device's exponentials
    exp32 = lambda v: np.exp(v.astype(np.float64)).astype(f)
    T, r, d, o = np.ones(R, f), np.zeros((R, 3), f), np.zeros(R, f), np.zeros(R, f)
    alive = N > 0
    stop = np.full(R, -1, np.int64)
    for k in range(int(N.max(initial=0))):
        has = k < N
        act = alive & has
        if not act.any():
            break
        slot = np.where(has, (row0 + k) * 64 + lane, 0)
        tslot = np.where(has, ((lt * arena_rows + k) << 6) + lane, 0) if arena_rows > 0 else slot
        v = packed[slot].astype(f)
        h0, c, t = np.where(act, v[:, 0], f(0)), v[:, 1:], ts[tslot]
        last = k + 1 >= N
        with np.errstate(over='ignore', invalid='ignore'):
            dt = np.maximum(dt_min, np.minimum(t * esf, dt_max))
            a = f(1) - exp32(-(exp32(h0) * dt))
            w = a * T
            r_new = np.stack([fma(w, c[:, i], r[:, i]) for i in range(3)], axis=1)
            d_new = d + w * (dt if mutant == 'depth_dt' else t)
            o_new = o + w
            T_new = T * (f(1) - a)
        m = act & ~last if mutant == 'skip_last' else act
        r, d, o, T = np.where(m[:, None], r_new, r), np.where(m, d_new, d), np.where(m, o_new, o), np.where(m, T_new, T)
        done = act & (((T < thr) if mutant == 'strict_threshold' else (T <= thr)) | last)
        stop = np.where(done, k, stop)
        alive = alive & ~done
    al = np.minimum(np.maximum(o, f(0)), f(1))
    Tr = f(1) - al
    rgb = np.stack([np.minimum(np.maximum(fma(Tr, np.broadcast_to(bg[i], Tr.shape), r[:, i]), f(0)), f(1)) for i in range(3)], axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        depth = np.where(Tr < f(1), d / al, f(0)).astype(f)
    return dict(pix=pix[inside], rgb=rgb[inside], alpha=al[inside], depth=depth[inside], stop=stop, n=N, inside=inside)


# ------------------------------------------------------------------------------------------------ synthetic tiled frames
WIDTH, HEIGHT = 19, 13        # 3 x 2 tiles; the right column and the bottom row of tiles are partly outside
N_TILES = 6
DEFAULTS = dict(width=WIDTH, height=HEIGHT, cascades=1, esf=0.0, grid_size=128, max_samples=1024, T_threshold=1e-4, bg3=(0.2, 0.5, 0.7))


def _layout(rng):
    """Per-lane counts from COUNTS (0 outside the image, like the count pass writes them), rows per tile = its longest ray."""
    _, _, pix = _geometry(WIDTH, HEIGHT, 0, N_TILES)
    cnt = np.where(pix >= 0, rng.choice(COUNTS, size=N_TILES * 64), 0).astype(np.int32)
    rows = cnt.reshape(N_TILES, 64).max(axis=1)
    tile_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return cnt, tile_off


def _frame(cnt, tile_off, h0, rgb, t, **params):
    """Scatter per-ray (R, K) sample arrays into the tiled layout.  Slots no ray owns hold NaN values and t = -1 (holes)."""
    rows = int(tile_off[-1])
    packed = np.full((rows * 64, 4), np.nan, np.float16)
    ts = np.full(rows * 64, -1.0, np.float32)
    R, K = h0.shape
    q, k = np.nonzero(np.arange(K)[None, :] < cnt[:, None])
    slot = (tile_off[q // 64].astype(np.int64) + k) * 64 + (q % 64)
    packed[slot, 0] = h0[q, k].astype(np.float16)
    packed[slot, 1:] = rgb[q, k].astype(np.float16)
    ts[slot] = t[q, k].astype(np.float32)
    case = dict(DEFAULTS)
    case.update(params)
    case.update(packed=packed, ts=ts, ray_cnt=cnt, tile_off=tile_off, tile_begin=0, n_tiles=N_TILES, row_capacity=0, arena_rows=0)
    for key in ('packed', 'ts', 'ray_cnt', 'tile_off'):
        case[key].setflags(write=False)
    return case


def _linear_t(R, K, max_samples):
    dt_min = np.float32(SQRT3) / np.float32(max_samples)
    return (np.float32(0.2) + np.arange(K, dtype=np.float32)[None, :] * dt_min) * np.ones((R, 1), np.float32)


def plain(seed):
    """esf = 0, one cascade: h0 ~ N(-1, 2) as fp16, colours in [0, 1], t from 0.2 in steps of dt_min."""
    rng = np.random.default_rng(seed)
    cnt, tile_off = _layout(rng)
    R, K = len(cnt), max(COUNTS)
    return _frame(cnt, tile_off, rng.normal(-1.0, 2.0, (R, K)), rng.random((R, K, 3)), _linear_t(R, K, 1024))


def saturating(seed):
    """h0 up to +9 around a level drawn per ray: most rays stop early, at different samples within a tile."""
    rng = np.random.default_rng(seed)
    cnt, tile_off = _layout(rng)
    R, K = len(cnt), max(COUNTS)
    h0 = np.minimum(rng.uniform(3.0, 9.5, (R, 1)) + rng.normal(0.0, 1.5, (R, K)), 9.0)
    return _frame(cnt, tile_off, h0, rng.random((R, K, 3)), _linear_t(R, K, 1024))


def step_regimes(seed, esf):
    """Three cascades, grid 128, 1024 samples; t from 0.2 to 30 so that the lower clamp, t * esf and the upper clamp sqrt3 * 2 * 3 / 128 all
    hold samples (esf = 1/256: lower clamp below t = 0.433, upper from t = 20.8; esf = 1/32: upper clamp from t = 2.6)."""
    rng = np.random.default_rng(seed)
    cnt, tile_off = _layout(rng)
    R, K = len(cnt), max(COUNTS)
    dt_min, dt_max = step_constants(3, 128, 1024)
    lo, hi = dt_min * 256, dt_max * 256
    which = rng.random((R, K))
    v = rng.random((R, K))
    t = np.where(which < 0.2, 0.2 + v * (lo - 0.2), np.where(which < 0.7, lo * (hi / lo) ** v, hi + v * (30.0 - hi)))
    t = np.sort(t.astype(np.float32), axis=1)
    # a ray's first cnt samples are what it owns: spread every ray over the whole range, not only rays of 70
    idx = np.minimum((np.arange(K)[None, :] * (K / np.maximum(cnt, 1)[:, None])).astype(np.int64), K - 1)
    t = np.take_along_axis(t, idx, axis=1)
    # densities that let rays reach the far samples: sigma dt stays small where dt is 50 times the lower clamp
    return _frame(cnt, tile_off, rng.normal(-3.0, 1.5, (R, K)), rng.random((R, K, 3)), t, cascades=3, esf=esf)


def extremes(seed, bg3):
    """`plain` with rays rewritten: single samples of h0 = -30 (a rounds to 0 in f32: the no-hit branch), h0 = +12 (a = 1), h0 = +89 (f32
    sigma = inf: expf overflows above 88.72) and h0 = 88.6875 (the largest fp16 below that point: the largest finite sigma, 3.3e38),
    colours of -0.25 and 1.5 (both rgb clamps), forty samples of a ~ 0.02.  Returns (case, marks): marks name the slots that were rewritten."""
    rng = np.random.default_rng(seed)
    cnt, tile_off = _layout(rng)
    cnt = cnt.copy()
    R, K = len(cnt), max(COUNTS)
    h0, rgb, t = rng.normal(-1.0, 2.0, (R, K)), rng.random((R, K, 3)), _linear_t(R, K, 1024)
    rays = np.nonzero(cnt > 0)[0]
    pick = rng.permutation(rays)
    marks = {}
    marks['no_hit'] = pick[:12]
    cnt[pick[:12]] = 1
    h0[pick[:12], 0] = -30.0
    marks['opaque'] = pick[12:24]                       # a = 1 at a sample drawn inside the ray
    for q in pick[12:24]:
        h0[q, rng.integers(0, cnt[q])] = 12.0
    marks['inf'] = pick[24:30]
    for j, q in enumerate(pick[24:30]):
        h0[q, min(j, cnt[q] - 1)] = 89.0
    marks['huge'] = pick[74:78]
    h0[pick[74:78], 0] = 88.6875
    marks['above_one'] = pick[30:50]
    rgb[pick[30:50]] = 1.5
    marks['below_zero'] = pick[50:70]
    rgb[pick[50:70]] = -0.25
    marks['forty'] = pick[70:74]
    cnt[pick[70:74]] = 40
    dt_min = step_constants(1, 128, 1024)[0]
    h0[pick[70:74], :] = np.log(-np.log1p(-0.02) / dt_min)
    rows = cnt.reshape(N_TILES, 64).max(axis=1)
    tile_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return _frame(cnt, tile_off, h0, rgb, t, bg3=bg3), marks


def tie(seed):
    """A constructed tie at the early-out: T_threshold = 1, and a third of the rays open with sigma = 0 (h0 = -inf in fp16: exp gives 0, the
    product 0, the exponential 1, every operation exact in f32 and f64).  T = 1 <= 1 after that sample: the ray stops there having
    composited nothing; every other ray stops after its first sample too.  `T < T_threshold` would walk on into the second sample."""
    rng = np.random.default_rng(seed)
    cnt, tile_off = _layout(rng)
    R, K = len(cnt), max(COUNTS)
    h0 = rng.normal(-1.0, 2.0, (R, K))
    h0[rng.random(R) < 1 / 3, 0] = -np.inf
    return _frame(cnt, tile_off, h0, rng.random((R, K, 3)), _linear_t(R, K, 1024), T_threshold=1.0)


def shard_of(case, tile_begin, n_tiles):
    """The arrays a shard's own count pass would produce: ray_cnt / tile_off / rows of the tiles [tile_begin, tile_begin + n_tiles) only."""
    off = case['tile_off'].astype(np.int64)
    r0, r1 = int(off[tile_begin]), int(off[tile_begin + n_tiles])
    out = dict(case)
    out.update(packed=case['packed'][r0 * 64:r1 * 64], ts=case['ts'][r0 * 64:r1 * 64], ray_cnt=case['ray_cnt'][tile_begin * 64:(tile_begin + n_tiles) * 64],
               tile_off=(off[tile_begin:tile_begin + n_tiles + 1] - r0).astype(np.int32), tile_begin=tile_begin, n_tiles=n_tiles)
    return out


def arena_of(case):
    """The same frame with `ts` in the count pass's arena: sample k of local tile lt in row lt * arena_rows + k, arena_rows = max_samples."""
    rows_per = case['max_samples']
    nt = case['n_tiles']
    arena = np.full(nt * rows_per * 64, -1.0, np.float32)
    off = case['tile_off'].astype(np.int64)
    for lt in range(nt):
        n = int(off[lt + 1] - off[lt])
        arena[lt * rows_per * 64:(lt * rows_per + n) * 64] = case['ts'][off[lt] * 64:off[lt + 1] * 64]
    out = dict(case)
    out.update(ts=arena, arena_rows=rows_per)
    return out


def capacity_of(case, tile=3):
    """row_capacity in the middle of `tile`'s rows."""
    off = case['tile_off'].astype(np.int64)
    out = dict(case)
    out['row_capacity'] = int(off[tile] + (off[tile + 1] - off[tile]) // 2)
    return out


ARG_NAMES = ('packed', 'ts', 'ray_cnt', 'tile_off', 'width', 'height', 'tile_begin', 'n_tiles', 'cascades', 'esf', 'grid_size', 'max_samples',
             'T_threshold', 'bg3', 'row_capacity', 'arena_rows')


def args_of(case):
    return [case[k] for k in ARG_NAMES]


BACKGROUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.2, 0.5, 0.7))
SHARDS = ((0, 6), (1, 2), (4, 2))
# seeds for which the f64 reference alone meets the cases' conditions (threshold rays <= 1 %, regime and stop shares, a tile with a ray of
# count 0 beside one of 70): tests/test_image_composite_ref_cpu.py asserts them
SEEDS = dict(plain=11, saturating=12, step_regimes=13, extremes=14, tie=15)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case dict, every generated case of the issue's table (built once, read-only)."""
    p = plain(SEEDS['plain'])
    out = {'plain': p, 'saturating': saturating(SEEDS['saturating']), 'tie': tie(SEEDS['tie'])}
    for esf, tag in ((1 / 256, '256'), (1 / 32, '32')):
        out[f'step_regimes_{tag}'] = step_regimes(SEEDS['step_regimes'], esf)
    for i, bg in enumerate(BACKGROUNDS):
        out[f'extremes_bg{i}'] = extremes(SEEDS['extremes'], bg)[0]
    for b, n in SHARDS:
        out[f'sharded_{b}_{n}'] = shard_of(p, b, n)
    out['arena'] = arena_of(p)
    out['capacity'] = capacity_of(p)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """composite_image_f64 with its budget for a named case (computed once, shared, read-only)."""
    ref = composite_image_f64(*args_of(cases()[name]), with_budget=True)
    for v in list(ref.values()) + list(ref['budget'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def assert_pixels_within_budget(got, ref, name):
    """Every pixel of got['rgb' / 'alpha' / 'depth'] (arrays in the order of ref['pix']) within ITS budget, none exempt; the worst one is reported.
    Returns {output: max err / budget}."""
    worst = {}
    for key in ('rgb', 'alpha', 'depth'):
        g, r, b = np.asarray(got[key], np.float64), np.asarray(ref[key], np.float64), np.asarray(ref['budget'][key], np.float64)
        assert g.shape == r.shape == b.shape, f'{name} {key}: shapes {g.shape}, {r.shape}, {b.shape}'
        assert np.isfinite(r).all() and np.isfinite(b).all() and (b >= 0).all(), f'{name} {key}: reference or budget is not finite'
        err = np.abs(g - r)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(err == 0, 0.0, err / b)
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)     # a NaN / inf of `got`, or an error where the budget is 0
        if ratio.size == 0:
            worst[key] = 0.0
            continue
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        if not ratio[i] <= 1.0:
            raise AssertionError(f'{name} {key}: pixel {int(ref["pix"][i[0]])} {i[1:]} got {float(g[i])!r} ref {float(r[i])!r} |err| {err[i]:.3e} budget {b[i]:.3e} '
                                 f'(err/budget {ratio[i]:.3g}; {int((ratio > 1).sum())} of {ratio.size} over)')
        worst[key] = float(ratio[i])
    return worst
