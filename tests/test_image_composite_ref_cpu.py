"""CPU: tests/image_composite_ref.py is trustworthy and has teeth.  Its float64 compositor is pinned against oracle.composite_test_fw (the C
restatement of volumerendering.cu:205-249) driven like the reference's alive-ray loop, an f32 emulation of the operation sequence must stay
inside the per-pixel budget on every case, wrong variants of that emulation must fall outside it, and the generated cases must contain what
they are meant to (threshold rays <= 1 %, step regimes, early stops).

Figures printed by this module (run with -s), SAFETY included.  Budget maxima per case:
    case                rgb        alpha      depth
    plain               6.43e-06   8.22e-06   1.02e-03      (rgb, alpha asserted below 1e-5)
    saturating          6.43e-06   7.96e-06   3.54e-06
    step_regimes 1/256  4.29e-06   1.14e-05   1.20e-02
    step_regimes 1/32   4.68e-06   1.10e-05   4.13e-03
    extremes, bg 0/1/c  1.03e-05 / 1.61e-05 / 1.08e-05   9.57e-06   0.4 (the undetermined depth of the h0 = -30 rays: max|t| + |depth|)
    tie                 2.21e-07   2.39e-07   0.317 (the same fallback on rays that composite a = 0 only)
The depth maxima sit on rays with alpha ~ 1e-4 (plain: one sample of sigma dt ~ 1e-4, where one ulp of the exponential is 1e-3 of alpha).
f32 emulation, max over pixels of |error| / budget: rgb 0.27 .. 0.45, alpha 0.23 .. 0.40, depth 0.008 .. 0.16 (0.5 on `extremes`: the
h0 = -30 rays, whose f32 pixel takes the no-hit branch).  The alpha figure is its floor: a ray of one thin sample carries the half ulp of a
correctly rounded exponential against a budget of 1.25 ulp.
The C oracle against the float64 reference, max |error| / budget, the same for chunks of 4, 64 and 1 to the digits shown: rgb 0.41 .. 0.50, alpha
0.23 .. 0.40, depth 0.02 .. 0.16 (its restart of T from 1 - opacity at every chunk stays inside the budget too).

`step_regimes` with esf = 1/32 cannot hold a sample on the LOWER clamp: t >= 0.2 gives t * esf >= 6.25e-3 > sqrt3 / 1024.  There the two regimes
that exist are asserted (>= 10 % each); all three at 1/256.
"""
import functools

import numpy as np
import pytest

import oracle
from tests import image_composite_ref as ic

ALL = tuple(ic.cases())
ORACLE_CASES = ('plain', 'saturating', 'step_regimes_256', 'step_regimes_32')


def _rays_of(case):
    """Ray-major (R, K) sample arrays of a case's rays that have samples, in slot order: sigma, rgb, dt, t as the f32 numbers an f32 caller hands
    to composite_test_fw (sigma = exp(h0) and the clamp rounded once), the counts and the slots."""
    f = np.float32
    cnt = case['ray_cnt'].astype(np.int64)
    q = np.nonzero(cnt > 0)[0]
    K = int(cnt.max())
    k = np.arange(K)[None, :]
    valid = k < cnt[q, None]
    slot = np.where(valid, (case['tile_off'][q // 64].astype(np.int64)[:, None] + k) * 64 + (q % 64)[:, None], 0)
    v = case['packed'][slot].astype(f)
    t = np.where(valid, case['ts'][slot], f(0))
    dt_min, dt_max = f(ic.SQRT3) / f(case['max_samples']), f(ic.SQRT3) * f(2) * f(case['cascades']) / f(case['grid_size'])
    dt = np.maximum(dt_min, np.minimum(t * f(case['esf']), dt_max))
    sigma = np.where(valid, np.exp(np.where(valid, v[..., 0], 0).astype(np.float64)), 0).astype(f)
    return sigma, np.where(valid[..., None], v[..., 1:], f(0)), dt, t, cnt[q], q


def _oracle_frame(case, chunk):
    """Renderer.py:104-138 on a case's samples: chunks of `chunk` samples per alive ray through oracle.composite_test_fw, the alive list carried
    over, then the finalisation in f32 numpy.  Returns the pixel arrays in the order of reference(...)['pix'] and, per slot, the chunk in which
    the ray left the alive list."""
    f = np.float32
    sigma, rgbs, dt, t, cnt, q = _rays_of(case)
    n = len(q)
    op, dp, col = np.zeros(n, f), np.zeros(n, f), np.zeros((n, 3), f)
    alive = np.arange(n, dtype=np.int64)
    left = np.full(len(case['ray_cnt']), -1, np.int64)
    for it in range(-(-int(cnt.max()) // chunk) + 1):
        if len(alive) == 0:
            break
        k = it * chunk + np.arange(chunk)[None, :]
        n_eff = np.clip(cnt[alive] - it * chunk, 0, chunk).astype(np.int32)
        kk = np.minimum(k, sigma.shape[1] - 1)
        take = lambda a: np.ascontiguousarray(a[alive[:, None], kk])
        before = alive.copy()
        oracle.composite_test_fw(take(sigma), take(rgbs), take(dt), take(t), alive, case['T_threshold'], n_eff, op, dp, col)
        gone = alive < 0
        left[q[before[gone]]] = it
        alive = alive[alive >= 0]
    assert len(alive) == 0
    bg = np.asarray(case['bg3'], f)
    alpha = np.clip(op, f(0), f(1))
    Tr = f(1) - alpha
    rgb = np.clip(col + Tr[:, None] * bg[None], f(0), f(1))
    with np.errstate(divide='ignore', invalid='ignore'):
        depth = np.where(Tr < f(1), dp / alpha, f(0))
    # scatter to the order of the reference's pixels (rays inside the image, slot order; rays without samples: background)
    _, _, pix = ic._geometry(case['width'], case['height'], case['tile_begin'], case['n_tiles'])
    inside = pix >= 0
    R = len(pix)
    full = dict(rgb=np.tile(np.clip(bg, 0, 1), (R, 1)), alpha=np.zeros(R, f), depth=np.zeros(R, f))
    full['rgb'][q], full['alpha'][q], full['depth'][q] = rgb, alpha, depth
    return {key: v[inside] for key, v in full.items()}, left


@pytest.mark.parametrize('chunk', [4, 64, 1])
@pytest.mark.parametrize('name', ORACLE_CASES)
def test_f64_reference_agrees_with_the_c_oracle(name, chunk):
    """What makes the reference trustworthy without a GPU.  Chunks of 4 and 64 as test_raymarching_test_and_composite_with_cascades_and_
    exponential_steps drives the oracle; a ray that saturates leaves the alive list in the chunk that holds its stop index (chunk 1: at that
    index), a ray that runs out of samples one round after its last one (n_eff = 0, volumerendering.cu:222-225)."""
    case, ref = ic.cases()[name], ic.reference(name)
    got, left = _oracle_frame(case, chunk)
    worst = ic.assert_pixels_within_budget(got, ref, f'{name} chunk {chunk}')
    print(f'\n{name} chunks of {chunk}: oracle err / budget {worst}')
    thr = float(np.float32(case['T_threshold']))
    has = (ref['n'] > 0) & ~ref['threshold'] & (np.abs(ref['T'] - thr) > ref['e_T'])
    stop, n = ref['stop'][has], ref['n'][has]
    saturated = ref['T'][has] <= thr
    assert ((stop == n - 1) | saturated).all()
    np.testing.assert_array_equal(left[has], np.where(saturated, stop // chunk, (n - 1) // chunk + 1))


@functools.lru_cache(maxsize=None)
def _emulation(name, mutant=None):
    return ic.composite_image_f32(*ic.args_of(ic.cases()[name]), mutant=mutant)


@pytest.mark.parametrize('name', ALL)
def test_f32_emulation_stays_inside_the_budget(name):
    ref = ic.reference(name)
    got = _emulation(name)
    worst = ic.assert_pixels_within_budget(got, ref, name)
    print(f'\n{name}: f32 emulation err / budget {worst}')
    off = ~ref['threshold']
    np.testing.assert_array_equal(got['stop'][off], ref['stop'][off])
    assert max(worst.values()) <= 0.6     # and not by a hair: SAFETY and the ulp granted to each exponential are unused by a correctly rounded one


MUTANTS = {'strict_threshold': ('tie',), 'depth_dt': ('plain', 'saturating', 'step_regimes_32'), 'no_dt_max': ('step_regimes_32', 'step_regimes_256'),
           'skip_last': ('plain', 'step_regimes_256', 'capacity', 'sharded_1_2'), 'scale_clamp': ('step_regimes_32',)}


@pytest.mark.parametrize('mutant,name', [(m, n) for m, names in MUTANTS.items() for n in names])
def test_wrong_compositors_fall_outside_the_budget(mutant, name):
    """The four edits the budget exists to catch (and the train march's `scale` in the upper clamp), applied to the emulation."""
    with pytest.raises(AssertionError, match='err/budget'):
        ic.assert_pixels_within_budget(_emulation(name, mutant), ic.reference(name), f'{name} {mutant}')


@pytest.mark.parametrize('name', ALL)
def test_case_conditions(name):
    case, ref = ic.cases()[name], ic.reference(name)
    has = ref['n'] > 0
    assert has.sum() > 40
    share = ref['threshold'][has].mean()
    bud = {k: float(v.max()) for k, v in ref['budget'].items()}
    print(f'\n{name}: rays with samples {int(has.sum())}, threshold rays {share:.4f}, budget maxima {bud}')
    assert share <= ic.THRESHOLD_RAY_CAP
    cnt = case['ray_cnt'].reshape(-1, 64)
    if case['n_tiles'] == ic.N_TILES:
        # every tile mixes lengths; at least one holds a ray of count 0 (inside the image) beside one of 70
        _, _, pix = ic._geometry(case['width'], case['height'], 0, ic.N_TILES)
        inside = (pix >= 0).reshape(-1, 64)
        assert all(len(np.unique(c[i])) >= 5 for c, i in zip(cnt, inside))
        assert any(((c == 0) & i).any() and (c == 70).any() for c, i in zip(cnt, inside))
    if name == 'plain':
        assert bud['alpha'] < ic.PLAIN_CEILING and bud['rgb'] < ic.PLAIN_CEILING
        assert set(np.unique(case['ray_cnt'])) == set(ic.COUNTS)
    if name == 'saturating':
        assert float(case['packed'][:, 0][~np.isnan(case['packed'][:, 0])].max()) == 9.0
        assert (ref['stop'][has] < ref['n'][has] - 1).mean() >= 0.30
        at8 = ref['at8'].reshape(-1, 64, 2)
        assert (at8[..., 0].any(axis=1) & at8[..., 1].any(axis=1)).any()     # a tile with stopped AND running lanes at sample 8
        stops = [np.unique(s[h]) for s, h in zip(ref['stop'].reshape(-1, 64), has.reshape(-1, 64))]
        assert all(len(s) >= 4 for s in stops)                                # ... which stop at different samples
    if name.startswith('step_regimes'):
        frac = ref['regimes'] / ref['regimes'].sum()
        upper = ic.step_constants(3, 128, 1024)[1]
        assert abs(upper - np.sqrt(3) * 2 * 3 / 128) < 1e-8 and case['cascades'] == 3
        if name.endswith('256'):
            assert (frac >= 0.10).all(), frac
        else:
            assert frac[0] == 0 and (frac[1:] >= 0.10).all(), frac      # t >= 0.2 cannot sit on the lower clamp at 1/32 (module docstring)
            t = case['ts'][case['ts'] > 0]
            assert ((t > 2.6) & (t < 20.0)).mean() > 0.2                # upper clamp at 1/32, t * esf at 1/256: what tells the two rules apart
        assert float(case['ts'].max()) > 29.0 and float(case['ts'][case['ts'] > 0].min()) < 0.21


def test_extremes_hold_what_they_promise():
    f = np.float32
    for i, bg in enumerate(ic.BACKGROUNDS):
        case, marks = ic.extremes(ic.SEEDS['extremes'], bg)
        ref, emu = ic.reference(f'extremes_bg{i}'), _emulation(f'extremes_bg{i}')
        where = lambda slots: np.searchsorted(np.nonzero(ref['inside'])[0], slots)      # slot -> row of the pixel arrays
        h0 = case['packed'][:, 0]
        assert (h0 == f(-30)).sum() >= 12 and (h0 == f(12)).sum() >= 12 and (h0 == f(89)).sum() >= 1
        with np.errstate(over='ignore'):       # expf overflows between the fp16 neighbours 88.6875 and 88.75; 89 lies above
            assert np.isfinite(np.exp(f(np.float16(88.6875)))) and np.isinf(np.exp(f(np.float16(88.75)))) and np.isinf(np.exp(f(89.0)))
        assert (h0 == np.float16(88.6875)).sum() >= 1
        # h0 = -30: a rounds to 0 in f32 -- the no-hit branch; the f64 reference sees alpha ~ 1.6e-16 and a depth it cannot vouch for
        p = where(marks['no_hit'])
        assert (emu['alpha'][p] == 0).all() and (emu['depth'][p] == 0).all() and (emu['rgb'][p] == np.clip(np.asarray(bg, f), 0, 1)).all()
        assert (ref['alpha'][p] < 1e-15).all() and (ref['budget']['depth'][p] >= ref['depth'][p]).all()
        # h0 = +12 / +89: the ray ends there with alpha = 1
        for key in ('opaque', 'inf', 'huge'):
            p = where(marks[key])
            assert (emu['alpha'][p] >= f(1) - f(2.0 ** -20)).all() and np.isfinite(emu['depth'][p]).all() and np.isfinite(ref['depth'][p]).all()
        assert (ref['stop'][marks['inf']] < ref['n'][marks['inf']] - 1).any()      # the f32 infinity sits inside a ray, not only at its end
        # both rgb clamps act
        hi, lo = where(marks['above_one']), where(marks['below_zero'])
        if min(bg) == 1:      # 1.5 o + (1 - o) > 1: the upper clamp on every such pixel of the white frame
            assert (ref['rgb'][hi] == 1.0).all() and (emu['rgb'][hi] == 1).all()
        if max(bg) == 0:      # -0.25 o < 0: the lower clamp on the black one
            assert (ref['rgb'][lo] == 0.0).all() and (emu['rgb'][lo] == 0).all()
        p = where(marks['forty'])
        assert (ref['n'][marks['forty']] == 40).all() and np.allclose(ref['alpha'][p], 1 - 0.98 ** 40, atol=2e-3)


def test_shards_arena_and_capacity_in_the_reference():
    full = ic.reference('plain')
    by_pix = {int(p): i for i, p in enumerate(full['pix'])}
    for b, n in ic.SHARDS:
        part = ic.reference(f'sharded_{b}_{n}')
        rows = [by_pix[int(p)] for p in part['pix']]
        for key in ('rgb', 'alpha', 'depth'):
            np.testing.assert_array_equal(part[key], full[key][rows])
        tiles_x = 3
        assert set((part['pix'] // ic.WIDTH // 8) * tiles_x + (part['pix'] % ic.WIDTH) // 8) == set(range(b, b + n))
    arena = ic.reference('arena')
    for key in ('rgb', 'alpha', 'depth', 'stop'):
        np.testing.assert_array_equal(arena[key], full[key])
    # row_capacity in the middle of tile 3: earlier tiles unchanged, tile 3's rays cut to the rows that exist, later tiles composite nothing
    case, cap = ic.cases()['capacity'], ic.reference('capacity')
    off = case['tile_off'].astype(np.int64)
    rows_left = case['row_capacity'] - off[3]
    assert 0 < rows_left < off[4] - off[3]
    tile = np.repeat(np.arange(ic.N_TILES), 64)
    np.testing.assert_array_equal(cap['n'][tile < 3], full['n'][tile < 3])
    np.testing.assert_array_equal(cap['n'][tile == 3], np.minimum(full['n'][tile == 3], rows_left))
    assert (cap['n'][tile > 3] == 0).all() and (full['n'][tile > 3] > 0).any() and (cap['n'][tile == 3] < full['n'][tile == 3]).any()
    slot_of_row = np.nonzero(full['inside'])[0]
    early = tile[slot_of_row] < 3
    for key in ('rgb', 'alpha', 'depth'):
        np.testing.assert_array_equal(cap[key][early], full[key][early])
    late = tile[slot_of_row] > 3
    assert (cap['alpha'][late] == 0).all() and (cap['depth'][late] == 0).all()
    # a cut ray is the ray of its first rows_left samples: the same frame with the counts cut by hand
    cut = dict(ic.cases()['plain'])
    cut['ray_cnt'] = np.where(tile == 3, np.minimum(case['ray_cnt'], rows_left), np.where(tile > 3, 0, case['ray_cnt'])).astype(np.int32)
    by_hand = ic.composite_image_f64(*ic.args_of(cut))
    for key in ('rgb', 'alpha', 'depth', 'stop'):
        np.testing.assert_array_equal(cap[key], by_hand[key])
