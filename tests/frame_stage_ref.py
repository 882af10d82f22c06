"""A float64 restatement and per-element fp16 intervals for the two middle stages of the fused image frame (nerficg_amd/csrc/ngp_net.hip):
stage 3a, nrc_ngp_encode_samples (k_grid_encode<SRC_TILED>), and stage 3b, nrc_ngp_mlp_samples (k_ngp_mlp<SRC_TILED>); the array-input encoder
(k_grid_encode_pairs / k_grid_encode<SRC_ARRAYS>) is judged by the same encoder interval.  Plain module: no test functions.  Used by
tests/test_frame_stage_ref_cpu.py and tests/test_gpu_frame_stages.py.

Positions (`slot_positions`)
---------
Slot i of the tiled layout is row i >> 6, lane i & 63, of the FRAME; its ray is row_tile[row] * 64 + lane, with origin and direction in the per-tile SoA
ray_od[tile][6][64].  A row with row_tile < 0 belongs to a finished tile (state -1: nothing of it is read or written), a slot with t < 0 is a hole (state 0).
t is read at the slot itself or, in the arena form, at arena row tile * arena_rows + (row - arena_tile_off[tile]).  fetch_pos<SRC_TILED>:
    p = (o + t d) - mn,   then p / sz unless sz == (1, 1, 1)                    -- one f32 rounding per operation
restated with numpy float32 operations, which round the same way (IEEE round to nearest even, no contraction).

Cell and fraction (`cells`)
-----------------
fx = fmaf(scale, p, 0.5) is ONE rounding of the exact value, cell = floor(fx), fraction = fx - floor(fx) (exact in f32).  scale and p are f32 numbers, so
scale * p is exact in float64 (24 + 24 bits); where the float64 sum with 0.5 is exact too (TwoSum's error term is zero: all but positions next to 0) its
one rounding to f32 is the fmaf; for the others the exact value is formed in `fractions` arithmetic and rounded once to f32 by integer division.  For
multiples of 2^-20 in [0, 1] this is input_grad_ref._cells (tests/test_frame_stage_ref_cpu.py).

Features (`grid_features`) and their bound
--------
Float64 from input_grad_ref's corner values: f = sum_k w_k v_k over the eight corners (k: x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2)), and alongside
A = sum_k |w_k v_k|.  The kernel (grid_cell / grid_level_features*) rounds each weight three times -- 1 - w, wx * wy, the product with wz -- and adds the
eight addends in eight fmaf, each rounding at most u A, u = 2^-24:
    e = 13 u A          3 + 8, plus 2 for the second-order terms and for the restatement's own float64 rounding.
The device value must lie in [fp16(f - e), fp16(f + e)] (mlp_ref._conv_bound's rule: rounding is monotone).  For almost every element the interval is
ONE fp16 number and the check is equality of bits; an element whose interval holds more is `ambiguous` -- the tests cap their share.
No measured constant, no tensor maximum and no excluded element enter.

Layout (`unpack_features` / `pack_features`)
------
Fragment-major, as documented at k_grid_encode: the 16-byte vector [((j >> 5) * 4 + ((g + (j >> 5)) & 3)) * 32 + (j & 31)] holds levels 4g .. 4g + 3
(two fp16 features each) of slot j of the chunk.

MLP stage (`mlp_stage`)
---------
    h   = density net (one hidden layer, 16 outputs, no activation) of the 32 features              -> fp16
    rgb = colour net (two hidden layers, sigmoid) of [fp16(SH4(fp16(d * 0.5 + 0.5) * 2 - 1)) | h]    -> fp16, columns 0..2
    record = (h[0], r, g, b)
mlp_ref.forward restates both; mlp_ref.forward_budget carries the bounds: the density net from E_X (0 when the inputs are the feature buffer the DEVICE
wrote, so that each stage is judged on its own), its output bound and mlp_ref.sh_input_bound as E_X of the colour net.  h[0] must lie in the conversion
interval, rgb in mlp_ref's faithful-rounding interval of the sigmoid, which tolerates any f32 sigmoid error below half an fp16 ulp -- no figure for the
kernel's fast_sigmoid is assumed.  An rgb element is `ambiguous` when its interval is wider than the neighbour pair of the restated sigmoid, an h[0]
element when its interval holds more than one number.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import oracle
from tests import input_grad_ref as igr
from tests import mlp_ref

U = 2.0 ** -24
ENC_C = 13
F32 = np.float32
SHIPPED = igr.grid_cfg(16, 2)
SMALL_TABLE = igr.grid_cfg(16, 2, log2_hashmap_size=14)     # two dense levels, fourteen hashed ones of 2^14 entries
UNIT_BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
DIV_BOX = ((-1.5, -2.0, -0.75), (3.0, 4.0, 1.5))            # the division path; 3 and 1.5 are no powers of two


def grid_kw(cfg) -> dict:
    """keyword arguments of the oracle's grid functions"""
    return {k: cfg[k] for k in ('n_levels', 'log2_hashmap_size', 'base_resolution', 'per_level_scale')}


# ---- positions --------------------------------------------------------------------------------------------------------------------------------------------
def slot_positions(ts, row_tile, ray_od, box, first_row: int, n_rows: int, arena_tile_off=None, arena_rows: int = 0) -> dict:
    """The chunk's n_rows * 64 slots: pos (n,3) f32 (zero where state <= 0), state (n,) 1 sample / 0 hole / -1 row of a finished tile, ray (n,) index of
    the slot's ray (tile * 64 + lane), tile (n,)."""
    ts, row_tile = np.asarray(ts, F32).reshape(-1), np.asarray(row_tile, np.int64)
    ray_od = np.asarray(ray_od, F32).reshape(-1, 6, 64)
    mn, sz = np.asarray(box[0], F32), np.asarray(box[1], F32)
    i = first_row * 64 + np.arange(n_rows * 64, dtype=np.int64)
    row, lane = i >> 6, i & 63
    rt = row_tile[row]
    done = rt < 0
    tile = np.where(done, -1 - rt, rt)
    if arena_rows > 0:
        idx = ((tile * arena_rows + (row - np.asarray(arena_tile_off, np.int64)[tile])) << 6) + lane
    else:
        idx = i
    t = ts[np.where(done, 0, idx)]
    state = np.where(done, -1, np.where(t < 0, 0, 1))
    o, d = ray_od[tile, 0:3, lane], ray_od[tile, 3:6, lane]      # (n,3) each
    p = (o + t[:, None] * d) - mn
    if np.any(sz != F32(1.0)):
        p = p / sz
    assert p.dtype == F32
    return dict(pos=np.where(state[:, None] > 0, p, F32(0.0)), state=state, ray=tile * 64 + lane, tile=tile)


# ---- cell and fraction ------------------------------------------------------------------------------------------------------------------------------------
def _round_f32(v: Fraction) -> float:
    """the f32 number nearest to v, ties to even (normal and subnormal range; |v| stays far below the overflow threshold here)"""
    if v == 0:
        return 0.0
    sign, v = (-1.0 if v < 0 else 1.0), abs(v)
    n, d = v.numerator, v.denominator
    e = n.bit_length() - d.bit_length()            # 2^(e-1) < v < 2^(e+1)
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1                                     # now 2^e <= v < 2^(e+1)
    q = max(e, -126) - 23                          # exponent of the last place
    k, r = divmod(n << max(-q, 0), d << max(q, 0))
    twice = 2 * r
    if twice > (d << max(q, 0)) or (twice == (d << max(q, 0)) and (k & 1)):
        k += 1
    return sign * float(np.ldexp(float(k), q))     # k <= 2^24: exact


def fma_half(scale, x):
    """fmaf(scale, x, 0.5f) for ANY finite f32 x: one rounding of the exact value."""
    x = np.asarray(x, F32)
    a = np.float64(F32(scale)) * x.astype(np.float64)          # exact: 24 x 24 bits
    s = a + 0.5
    bb = s - a
    err = (a - (s - bb)) + (0.5 - bb)                          # TwoSum: s + err == a + 0.5 exactly
    out = s.astype(F32)                                        # one rounding where err == 0
    odd = np.flatnonzero(err.reshape(-1) != 0.0)
    if odd.size:
        flat, xs = out.reshape(-1), x.reshape(-1)
        vals, inv = np.unique(xs[odd], return_inverse=True)
        sc, half = Fraction(float(F32(scale))), Fraction(1, 2)
        exact = np.array([_round_f32(sc * Fraction(float(v)) + half) for v in vals], F32)
        flat[odd] = exact[inv]
        out = flat.reshape(x.shape)
    return out


def cells(x, scale, half: bool = True):
    """(cell (M,3) uint32, fraction (M,3) float64) of ANY finite f32 positions at a level: grid_cell's chain.  half=False: a deliberately wrong chain
    without the + 0.5 (tests/test_frame_stage_ref_cpu.py shows that the judge notices)."""
    x = np.asarray(x, F32)
    fx = fma_half(scale, x) if half else (F32(scale) * x)
    fl = np.floor(fx)
    return fl.astype(np.int32).astype(np.uint32), (fx - fl).astype(np.float64)     # (uint32_t)(int32_t) as in the kernel; fx - fl is exact in f32


# ---- features ---------------------------------------------------------------------------------------------------------------------------------------------
CORNERS = tuple(range(8))
SWAP_67 = (0, 1, 2, 3, 4, 5, 7, 6)


def grid_features(x, table, cfg, half: bool = True, corners=CORNERS) -> dict:
    """x (M,3) f32, any finite values inside the box; table (entries, 2) fp16-representable.  Returns f (M,32) float64 features, column level * 2 + c,
    A (M,32) = sum |w_k v_k|, lo / hi (M,32) the fp16 interval of the device value, cell (levels, M, 3) uint32.  `half`, `corners`: wrong encoders."""
    x = np.asarray(x, F32)
    _, offsets, scales, res = igr._layout(cfg)
    t64 = np.asarray(table, np.float64)
    F, L = t64.shape[1], cfg['n_levels']
    f, A = np.zeros((x.shape[0], L * F)), np.zeros((x.shape[0], L * F))
    cell_all = np.zeros((L, x.shape[0], 3), np.uint32)
    for l in range(L):
        cell, w1 = cells(x, scales[l], half)
        cell_all[l] = cell
        v = igr._corner_values(cell, t64, int(offsets[l]), int(res[l]), int(offsets[l + 1] - offsets[l]))
        w = np.stack([1.0 - w1, w1])   # [0 / 1][M][axis]
        for k in range(8):
            wk = w[k & 1, :, 0] * w[(k >> 1) & 1, :, 1] * w[k >> 2, :, 2]
            term = wk[:, None] * v[corners[k]]
            f[:, l * F:(l + 1) * F] += term
            A[:, l * F:(l + 1) * F] += np.abs(term)
    e = ENC_C * U * A
    return dict(f=f, A=A, e=e, lo=mlp_ref.h16(f - e), hi=mlp_ref.h16(f + e), cell=cell_all, x=x)


def ambiguous_share(lo, hi, rows=None) -> float:
    """share of the judged elements whose interval holds more than one fp16 number"""
    lo, hi = (lo, hi) if rows is None else (lo[rows], hi[rows])
    return float(np.mean(lo != hi)) if lo.size else 0.0


def judge_features(got, ref, rows=None, slots=None):
    """got (M,32): device features of the rows of ref (or of ref's rows `rows`).  Returns (elements outside their interval, report): the report names the
    worst element (slot, level, feature, device value, interval), its position and cell, and the count."""
    got = np.asarray(got, np.float64)
    sel = np.arange(ref['f'].shape[0]) if rows is None else np.asarray(rows)
    lo, hi, f = ref['lo'][sel], ref['hi'][sel], ref['f'][sel]
    with np.errstate(invalid='ignore'):
        bad = ~((got >= lo) & (got <= hi))
    n_bad = int(bad.sum())
    if n_bad == 0:
        return 0, ''
    with np.errstate(invalid='ignore'):
        dist = np.where(bad, np.maximum(np.maximum(lo - got, got - hi), 0.0), 0.0)
    dist = np.where(bad & ~np.isfinite(dist), np.inf, dist)
    r, c = np.unravel_index(int(np.argmax(dist)), dist.shape)
    level, feat = c // 2, c % 2
    slot = int(sel[r]) if slots is None else int(np.asarray(slots)[r])
    return n_bad, (f'{n_bad} of {bad.size} elements outside their interval; worst: slot {slot} level {level} feature {feat}: device {got[r, c]!r}, '
                   f'interval [{lo[r, c]!r}, {hi[r, c]!r}], float64 {f[r, c]!r} +- {ref["e"][sel[r], c]:.3e}; position {ref["x"][sel[r]].tolist()!r}, '
                   f'cell {ref["cell"][level, sel[r]].tolist()}')


def error_ratio(got, ref, rows=None) -> float:
    """largest |got - f| / e of UNROUNDED f32 features `got` (an emulation of the kernel's chain) over the elements with e > 0"""
    sel = slice(None) if rows is None else rows
    f, e = ref['f'][sel], ref['e'][sel]
    err = np.abs(np.asarray(got, np.float64) - f)
    assert np.all(err[e == 0] == 0)
    return float(np.max(np.where(e > 0, err / np.where(e > 0, e, 1.0), 0.0), initial=0.0))


def emulate_f32(x, table, cfg):
    """the kernel's own chain in f32, not rounded to fp16: weights 1 - w, wx * wy, (wx wy) * wz, then acc = fmaf(w_k, v_k, acc) over k = 0 .. 7 from 0 (each
    fmaf as one rounding of the float64 value: products of an f32 and an fp16 number and the sum with an f32 are far inside 53 bits except for a
    double rounding that 2^-29 of an ulp decides)"""
    x = np.asarray(x, F32)
    _, offsets, scales, res = igr._layout(cfg)
    t64 = np.asarray(table, np.float64)
    out = np.zeros((x.shape[0], cfg['n_levels'] * 2), F32)
    for l in range(cfg['n_levels']):
        cell, w1 = cells(x, scales[l])
        v = igr._corner_values(cell, t64, int(offsets[l]), int(res[l]), int(offsets[l + 1] - offsets[l]))
        w1 = w1.astype(F32)
        w = np.stack([F32(1.0) - w1, w1])
        acc = np.zeros((x.shape[0], 2), F32)
        for k in range(8):
            wk = (w[k & 1, :, 0] * w[(k >> 1) & 1, :, 1]) * w[k >> 2, :, 2]
            acc = (wk.astype(np.float64)[:, None] * v[k] + acc.astype(np.float64)).astype(F32)
        out[:, 2 * l:2 * l + 2] = acc
    return out


# ---- layout -----------------------------------------------------------------------------------------------------------------------------------------------
def _vector_index(n_slots: int):
    j = np.arange(n_slots, dtype=np.int64)
    g = np.arange(4, dtype=np.int64)[None, :]
    return ((j[:, None] >> 5) * 4 + ((g + (j[:, None] >> 5)) & 3)) * 32 + (j[:, None] & 31)      # (n, 4): the vector of level group g of slot j


def unpack_features(buffer, n_slots: int):
    """buffer: the feature buffer as raw bytes / fp16 (at least ceil(n_slots / 32) * 2048 bytes).  Returns (n_slots, 32) float16, column level * 2 + c."""
    vec = np.ascontiguousarray(buffer).reshape(-1).view(np.float16).reshape(-1, 8)
    return vec[_vector_index(n_slots)].reshape(n_slots, 32)


def pack_features(feat, fill=0.0):
    """(n, 32) fp16 features -> the fragment-major buffer, (ceil(n / 32) * 128, 8) float16; the slots behind n hold `fill`."""
    feat = np.asarray(feat, np.float16)
    n = feat.shape[0]
    vec = np.full(((n + 31) // 32 * 128, 8), fill, np.float16)
    vec[_vector_index(n)] = feat.reshape(n, 4, 8)
    return vec


# ---- MLP stage --------------------------------------------------------------------------------------------------------------------------------------------
def sigmoid64(z):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def mlp_stage(features16, dirs, Wd, Wc, E_X=None) -> dict:
    """features16 (M,32) fp16 values (the encoder's output), dirs (M,3) f32 ray directions, Wd / Wc the flat fp16-representable weights of the density
    net [W0 (64,32) | Wout (16,64)] and the colour net [W0 (64,32) | W1 (64,64) | Wout (16,64)].  Returns the (M,4) record (h0, r, g, b): ref (restated),
    lo / hi (interval of the device value), ambiguous (M,4) bool."""
    X = np.asarray(features16, np.float64)
    fd = mlp_ref.forward_budget(X, Wd, 1, 0, E_X=E_X)
    h, (hlo, hhi) = fd['out_ref'], fd['out']
    E_h = np.maximum(np.abs(hlo - h), np.abs(hhi - h))
    d = np.asarray(dirs, F32)
    d01 = (d * F32(0.5) + F32(0.5)).astype(np.float16)                  # the kernel's two f32 operations, then the fp16 conversion
    Xc = np.concatenate([mlp_ref.h16(mlp_ref.sh4_f64(d01)), h], axis=1)
    E = mlp_ref.sh_input_bound(d01, Xc)
    E[:, 16:] = E_h
    fc = mlp_ref.forward_budget(Xc, Wc, 2, 1, E_X=E)
    s = sigmoid64(fc['fw']['Zout'][:, :3])
    pair_lo, pair_hi = mlp_ref.h16_down(s), mlp_ref.h16_up(s)
    lo = np.concatenate([hlo[:, :1], fc['out'][0][:, :3]], axis=1)
    hi = np.concatenate([hhi[:, :1], fc['out'][1][:, :3]], axis=1)
    ref = np.concatenate([h[:, :1], fc['out_ref'][:, :3]], axis=1)
    amb = np.concatenate([hlo[:, :1] != hhi[:, :1], (lo[:, 1:] != pair_lo) | (hi[:, 1:] != pair_hi)], axis=1)
    return dict(ref=ref, lo=lo, hi=hi, ambiguous=amb, h=h, h_iv=(hlo, hhi), zc=fc['fw']['Zout'][:, :3])


def judge_records(got, ref, rows, slots=None):
    """got (len(rows),4) device records of ref's rows `rows`.  Returns (elements outside their interval, report)."""
    got, rows = np.asarray(got, np.float64), np.asarray(rows)
    lo, hi = ref['lo'][rows], ref['hi'][rows]
    with np.errstate(invalid='ignore'):
        bad = ~((got >= lo) & (got <= hi))
    n_bad = int(bad.sum())
    if n_bad == 0:
        return 0, ''
    with np.errstate(invalid='ignore'):
        dist = np.where(bad, np.maximum(np.maximum(lo - got, got - hi), 0.0), 0.0)
    dist = np.where(bad & ~np.isfinite(dist), np.inf, dist)
    r, c = np.unravel_index(int(np.argmax(dist)), dist.shape)
    slot = int(rows[r]) if slots is None else int(np.asarray(slots)[r])
    return n_bad, (f'{n_bad} of {bad.size} record elements outside their interval; worst: slot {slot} element {"h0 r g b".split()[c]}: device {got[r, c]!r}, '
                   f'interval [{lo[r, c]!r}, {hi[r, c]!r}], restated {ref["ref"][rows[r], c]!r}')


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _levels(log2_hashmap_size: int):
    _, _, scales, res = igr._layout(igr.grid_cfg(16, 2, log2_hashmap_size=log2_hashmap_size))
    return [(float(s), int(r)) for s, r in zip(scales, res)]


@functools.lru_cache(maxsize=None)
def special_values(log2_hashmap_size: int = 19):
    """coordinates at which the cell or a weight of a level steps or sits in the middle, for ALL 16 levels: k / scale and (k +- 0.5) / scale for cells at
    both ends and in the middle of the level, the f32 neighbours of each on either side, and 0, 1, 1 - ulp"""
    vals = [0.0, 1.0]
    for scale, res in _levels(log2_hashmap_size):
        for k in sorted({0, 1, 2, res // 2, res // 2 + 1, res - 3, res - 2, res - 1, int(scale)}):
            vals += [v for v in (k / scale, (k - 0.5) / scale, (k + 0.5) / scale) if 0.0 <= v <= 1.0]
    vals = np.asarray(vals, F32)
    out = np.unique(np.clip(np.concatenate([vals, np.nextafter(vals, F32(-1)), np.nextafter(vals, F32(2))]), 0.0, 1.0))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def special_positions(log2_hashmap_size: int = 19, m: int = 2048, seed: int = 17):
    """(m, 3) f32: every special value on every axis at least once, 0 / 1 / 1 - ulp triples, random triples of special values behind them"""
    vals = special_values(log2_hashmap_size)
    assert m >= len(vals) + 8
    rng = np.random.default_rng(seed)
    x = rng.choice(vals, size=(m, 3)).astype(F32)
    for axis in range(3):
        x[:len(vals), axis] = np.roll(vals, 7 * axis)
    x[len(vals):len(vals) + 3] = np.array([0.0, 1.0, np.nextafter(F32(1), F32(0))], F32)[:, None]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def special_tile(log2_hashmap_size: int = 19, seed: int = 5) -> dict:
    """one ray tile of 16 rows (1 024 slots) in the unit box: ray r starts on the plane (its axis r % 3) = 0 with special values on the other two axes and
    runs along that axis with d = 1, so p = o + t d is exact and a special t puts all three coordinates on special values (the construction of
    tests/test_gpu_encoder_vertex_view.py::ray_tile, with the special values of all 16 levels)"""
    rows, n = 16, 1024
    vals = special_values(log2_hashmap_size)
    ends = np.array([0.0, 1.0, np.nextafter(F32(1), F32(0))], F32)
    assert 500 < len(vals) < 900 and vals[0] == ends[0] and vals[-1] == ends[1] and vals[-2] == ends[2], len(vals)
    rng = np.random.default_rng(seed)
    o = rng.choice(vals, size=(64, 3)).astype(F32)
    for i, e in enumerate(ends):                            # rays 3 .. 11: the two axes across the ray on an end value
        o[3 + 3 * i:6 + 3 * i] = e
    d = np.zeros((64, 3), F32)
    o[np.arange(64), np.arange(64) % 3] = 0.0
    d[np.arange(64), np.arange(64) % 3] = 1.0
    ts = rng.choice(vals, size=n).astype(F32)
    ts[:len(vals)] = vals                                   # every special value at least once
    holes = np.flatnonzero(rng.random(n) < 0.1)
    ts[holes[holes >= len(vals)]] = -1.0
    for i, e in enumerate(ends):                            # rows 13 .. 15, rays 0 .. 2 (one per axis): the axis along the ray on an end value
        ts[64 * (13 + i):64 * (13 + i) + 3] = e
    ray_od = np.concatenate([o.T, d.T]).reshape(1, 6, 64).astype(F32)
    frame = dict(ts=ts, row_tile=np.zeros(rows, np.int32), ray_od=ray_od, box=UNIT_BOX, first_row=0, n_rows=rows, frame_rows=rows, n_ray_tiles=1,
                 arena_tile_off=None, arena_rows=0)
    sp = slot_positions(ts, frame['row_tile'], ray_od, UNIT_BOX, 0, rows)
    live = sp['state'] > 0
    assert (~live).sum() > 20 and np.array_equal(sp['pos'][live], (o[np.arange(n) % 64] + ts[:, None] * d[np.arange(n) % 64])[live])
    for axis in range(3):
        assert all((sp['pos'][live, axis] == e).any() for e in ends), axis
        assert np.isin(vals, sp['pos'][live]).all()
    return _freeze(frame)


GENERAL_ROW_TILE = (2, 0, 1, 1, 0, 2, 2, 0, 1, 0, -2, 2, 1, 0, 0, 2, 1, 2, 0)      # 19 rows of three ray tiles; row 10 belongs to the finished tile 1


@functools.lru_cache(maxsize=None)
def general_frame(form: str = 'compact', seed: int = 23) -> dict:
    """three ray tiles in 19 rows (1 216 slots: the last block of 1 024 is partial), rows dealt to the tiles in an irregular order, one row of a finished
    tile; oblique unit directions, random origins and t, DIV_BOX.  Slots whose restated position leaves [0, 1]^3 are holes, 4 % more at random.
    form: 'compact' (first_row 0), 'shifted' (the same 19 rows as rows 3 .. 21 of a 22-row frame), 'arena' (t read from an arena)."""
    rows, nt = len(GENERAL_ROW_TILE), 3
    rng = np.random.default_rng(seed)
    mn, sz = np.asarray(DIV_BOX[0]), np.asarray(DIV_BOX[1])
    entry = mn + sz * rng.uniform(0.05, 0.95, size=(nt * 64, 3))
    d = rng.normal(size=(nt * 64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(np.abs(d) < 0.05, 0.05, d)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    back = rng.uniform(5.5, 7.0, size=(nt * 64, 1))            # (the box's diagonal is 5.2: every origin lies outside it)
    o = (entry - back * d).astype(F32)
    d = d.astype(F32)
    with np.errstate(divide='ignore'):
        t0, t1 = (mn - o) / d, (mn + sz - o) / d
    tmin, tmax = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    assert np.all(tmin < tmax) and np.all(tmin > 0)
    row_tile = np.asarray(GENERAL_ROW_TILE, np.int32)
    tile = np.where(row_tile < 0, -1 - row_tile, row_tile)
    ray = (tile[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    lam = rng.uniform(0.002, 0.998, size=rows * 64)
    ts = (tmin[ray] + lam * (tmax - tmin)[ray]).astype(F32)
    ray_od = np.concatenate([o.reshape(nt, 64, 3).transpose(0, 2, 1), d.reshape(nt, 64, 3).transpose(0, 2, 1)], axis=1).astype(F32)    # [tile][6][64]
    pos = slot_positions(ts, tile, ray_od, DIV_BOX, 0, rows)['pos']     # (every row as a live one: the finished row keeps real t)
    outside = np.any((pos < 0) | (pos > 1), axis=1)
    ts[outside | (rng.random(rows * 64) < 0.04)] = -1.0
    frame = dict(ts=ts, row_tile=row_tile, ray_od=ray_od, box=DIV_BOX, first_row=0, n_rows=rows, frame_rows=rows, n_ray_tiles=nt, arena_tile_off=None,
                 arena_rows=0)
    if form == 'shifted':
        lead = 3
        head_ts = rng.uniform(0.0, 4.0, size=lead * 64).astype(F32)
        frame.update(ts=np.concatenate([head_ts, ts]), row_tile=np.concatenate([np.array([1, 2, 0], np.int32), row_tile]), first_row=lead,
                     frame_rows=rows + lead)
    elif form == 'arena':
        # sample k = row - tile_off[tile] of the row's tile: tile_off = the tile's first row (rows 1, 2, 0), so k runs irregularly up to 18
        tile_off = np.array([int(np.flatnonzero(tile == t)[0]) for t in range(nt)] + [rows], np.int32)
        arena_rows = rows
        arena = np.full((nt, arena_rows, 64), np.nan, F32)          # (a slot nobody may read: NaN would make its features NaN)
        for r in range(rows):
            arena[tile[r], r - tile_off[tile[r]]] = ts[64 * r:64 * r + 64]
        frame.update(ts=arena.reshape(-1), arena_tile_off=tile_off, arena_rows=arena_rows)
    else:
        assert form == 'compact'
    sp = slot_positions(frame['ts'], frame['row_tile'], ray_od, DIV_BOX, frame['first_row'], rows, frame['arena_tile_off'], frame['arena_rows'])
    live = sp['state'] > 0
    assert np.all((sp['pos'][live] >= 0) & (sp['pos'][live] <= 1)) and np.array_equal(sp['state'][640:704], np.full(64, -1))
    assert live.sum() >= 0.9 * (rows - 1) * 64, live.mean()         # at least 90 % of the slots of the unfinished rows stay live
    return _freeze(frame)


def _freeze(frame):
    for a in frame.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return frame


def frame_slots(frame) -> dict:
    """slot_positions of a frame dict's chunk"""
    return slot_positions(frame['ts'], frame['row_tile'], frame['ray_od'], frame['box'], frame['first_row'], frame['n_rows'], frame['arena_tile_off'],
                          frame['arena_rows'])


def slot_dirs(frame, sp):
    """(n,3) f32 direction of every slot's ray"""
    od = np.asarray(frame['ray_od'], F32).reshape(-1, 6, 64)
    return od[sp['ray'] >> 6, 3:6, sp['ray'] & 63]


@functools.lru_cache(maxsize=None)
def uniform_table(log2_hashmap_size: int = 19, amp: float = 2.0, seed: int = 31, positive: bool = False):
    """(entries, 2) float32 holding random fp16 values, U(-amp, amp) (positive: their magnitudes)"""
    cfg = igr.grid_cfg(16, 2, log2_hashmap_size=log2_hashmap_size)
    rng = np.random.default_rng(seed)
    t = ((rng.random((igr.n_entries(cfg), 2), dtype=F32) * 2 - 1) * F32(amp)).astype(np.float16).astype(F32)
    t = np.abs(t) if positive else t
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def exact_model(seed: int = 0) -> dict:
    """mlp_ref.exact_case(grid=True)'s construction for the frame's two networks: ternary weights (the SH columns of the colour net's first layer zero) and a
    table that is constant per level, small integers -- every feature is that integer (an interpolation of equal values is the value to within a few
    2^-24, far inside half an fp16 ulp of an integer below 4), every sum of the networks is a sum of small integers: exact in f32 in any order.  h0 of a
    sample is ONE number, rgb the sigmoid of an integer.  Returns Wd, Wc, table (float32, fp16-representable), X (32,) the features of every sample, h0,
    z_rgb (3,) the colour head's pre-activations."""
    rng = np.random.default_rng([seed, 77])
    T = mlp_ref._ternary
    X = rng.integers(0, 4, size=(1, 32)).astype(np.float64)
    W0d, Wod = T(rng, (64, 32), 0.25), T(rng, (16, 64), 0.5)
    W0c = np.concatenate([np.zeros((64, 16)), T(rng, (64, 16), 0.25)], axis=1)
    W1c = T(rng, (64, 64), 0.12)
    Wd = np.concatenate([W0d.reshape(-1), Wod.reshape(-1)])
    fd = mlp_ref.forward(X, Wd, 1, 0)
    Xc = np.concatenate([np.full((1, 16), 0.25), fd['out']], axis=1)         # (SH columns: any value, their weights are zero)
    # the colour head's rows 0..2 are differences of two units of the last hidden layer, chosen so that the three pre-activations are distinct integers
    # in [-8, 8] without 0: sigmoids that neither are 0.5 nor saturate
    Woc = T(rng, (16, 64), 0.5)
    Woc[:3] = 0.0
    H = mlp_ref.forward(Xc, np.concatenate([W0c.reshape(-1), W1c.reshape(-1), Woc.reshape(-1)]), 2, 1)['H'][-1][0]
    diff = H[:, None] - H[None, :]
    seen = []
    for i, j in rng.permutation(np.argwhere((diff != 0) & (np.abs(diff) <= 8))):
        if diff[i, j] not in seen and len(seen) < 3:
            Woc[len(seen), i], Woc[len(seen), j] = 1.0, -1.0
            seen.append(diff[i, j])
    Wc = np.concatenate([W0c.reshape(-1), W1c.reshape(-1), Woc.reshape(-1)])
    fc = mlp_ref.forward(Xc, Wc, 2, 1)
    z = fc['Zout'][0, :3]
    assert fd['out'][0, 0] != 0 and len(seen) == 3 and np.array_equal(z, seen), (fd['out'][0, 0], z)
    assert all(bool(np.all(mlp_ref.h16(a) == a)) for a in fd['Z'] + [fd['Zout']] + fc['Z'])     # every converted value is an fp16 number already
    assert max(float(np.abs(a).max()) for a in fd['Z'] + [fd['Zout']] + fc['Z'] + [fc['Zout']]) < 2048      # integers far below 2^24: no f32 sum rounds
    _, offsets, _, _ = igr._layout(SHIPPED)
    table = np.zeros((int(offsets[-1]), 2), F32)
    for l in range(16):
        table[int(offsets[l]):int(offsets[l + 1])] = X[0, 2 * l:2 * l + 2]
    out = dict(Wd=Wd.astype(F32), Wc=Wc.astype(F32), table=table, X=X[0].copy(), h0=float(fd['out'][0, 0]), z_rgb=z.copy())
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def random_model_params(seed: int = 7, amps=(4.0, 0.4, 0.6)) -> dict:
    """the fp16 parameters of tests/test_gpu_frame_sh_hoist.py::random_model, drawn here without a device (the same generator, the same order: density
    net U(-0.4, 0.4), table U(-4, 4), colour net U(-0.6, 0.6)), as float32: Wd (3072), table (entries, 2), Wc (7168).  The GPU test asserts that the
    model's own fp16 copy holds these bits."""
    import torch
    g = torch.Generator().manual_seed(seed)
    u = lambda n, amp: ((torch.rand(n, generator=g) * 2 - 1) * amp).to(torch.float16).to(torch.float32).numpy()
    n_table = 2 * igr.n_entries(SHIPPED)
    out = dict(Wd=u(3072, amps[1]), table=u(n_table, amps[0]).reshape(-1, 2), Wc=u(7168, amps[2]))
    return _freeze(out)


def oracle_features(x, table, cfg, accumulate='float'):
    return oracle.grid_encode_fw(np.ascontiguousarray(x, F32), np.ascontiguousarray(table, F32), accumulate=accumulate, **grid_kw(cfg))
