"""CPU: tests/train_composite_ref.py is trustworthy and has teeth.  The cases hold what they promise (zero threshold rays, the constructed stop
positions, every ray length, a row count that is no multiple of 4); an np.float32 emulation of the wave-wide kernels stays inside every
budget; each wrong variant of it falls outside on a named case; the project's serial f32 C oracle -- a second implementation -- lies inside
the budgets of the new reference; the float64 closed form agrees with float64 autograd; the budgets cannot quietly grow.

Figures printed by this module (run with -s), SAFETY included.  Max |error| / budget over all elements:
    f32 emulation, train    opacity 0.26 .. 0.40, depth 0.26 .. 0.40, rgb 0.25 .. 0.40, ws 0.38 .. 0.40, dsigma 0.07 .. 0.18 (0.17 with NULL gradients),
                            drgb 0.38 .. 0.40 over plain / stops / thr0 / tie / extremes.  The ws figure is its floor: a thin sample carries the half
                            ulp of a correctly rounded exponential against a budget of 1.25 ulp.
    C oracle, train         plain: opacity 0.324, depth 0.323, rgb 0.363, ws 0.387, dsigma 0.072, drgb 0.387; stops: 0.367, 0.367, 0.367, 0.384, 0.080, 0.383
    C oracle, distortion    plain: loss 0.172, ws_incl 0.388, wts_incl 0.365, dws 0.383; stops: 0.111, 0.344, 0.391, 0.383
    f32 emulation, distortion   loss 0.11 .. 0.17, ws_incl 0.36 .. 0.39, wts_incl 0.36 .. 0.40, dws 0.38 .. 0.39 (plain / stops / equal_ts)
    inference, rows of 1 .. 130   C oracle: opacity 0.15 .. 0.32, depth 0.15 .. 0.32, rgb 0.18 .. 0.33; chunked emulation 0.09 .. 0.32, 0.12 .. 0.32, 0.17 .. 0.33
    march backward, serial f32    g_o 0.373, g_d 0.357 (0.208 without g_dirs)
    fused loss, f32 emulation     pixel 0.146, alpha 0.367, depth 0.114, loss2 < 0.001, dsigma 0.014, drgb 0.372
    mutants                 carry_reset on plain 1.0e5 (opacity), exclusive_prefix on plain 1.7e4 (dsigma), dws_sum_truncated on plain 6.8e3 (dsigma),
                            stop_not_composited on stops 4.5e6 (opacity), strict_threshold on tie: an error where the budget is 0 (13 rays),
                            count_includes_stop on stops: 24 of 45 counts off by one, every float output inside its budget
    closed form against autograd   dsigma <= 4.6e-16 of the bracket's operands, <= 8.5e-16 of the largest |dsigma|
    plain, largest budget / largest |value| of the ray   ws 3.11e-05, dsigma 1.78e-04, drgb 3.12e-05, opacity 8.10e-05, depth 9.00e-05, rgb 8.02e-05
"""
import functools

import numpy as np
import pytest

import oracle
from tests import train_composite_ref as tc

f32 = np.float32


def _dense32(case):
    d = tc._dense_case(case)
    return d, {k: d[k].astype(f32) for k in ('sigmas', 'rgbs', 'deltas', 'ts', 'gw')}


@functools.lru_cache(maxsize=None)
def _emulation(name, mutant=None, null_grads=False):
    """The f32 emulation of forward and backward on a case; the backward is fed the float64 forward rounded to f32, like the GPU test feeds it."""
    case, ref = tc.cases()[name], tc.train_reference(name, null_grads)
    d, v = _dense32(case)
    slot, M = d['ray_idx'], case['sigmas'].shape[0]
    fw = tc.emulate_fw(v['sigmas'], v['rgbs'], v['deltas'], v['ts'], d['N'], case['T_threshold'], mutant=mutant)
    n = len(slot)

    def by_slot(a):
        out = np.zeros((n,) + a.shape[1:], a.dtype)
        out[slot] = a
        return out
    got = dict(total=by_slot(fw['total']), opacity=by_slot(fw['opacity']), depth=by_slot(fw['depth']), rgb=by_slot(fw['rgb']),
               ws=tc.to_flat(fw['ws'].astype(np.float64), d['idx'], d['mask'], M))
    ws32 = tc.to_dense(ref['ws'], d['idx'], d['mask']).astype(f32)
    go, gd, gw = (None, None, None) if null_grads else (case['go'][slot], case['gd'][slot], v['gw'])
    ds, dr = tc.emulate_bw(v['sigmas'], v['rgbs'], v['deltas'], v['ts'], d['N'], case['T_threshold'], ws32, ref['opacity'][slot].astype(f32),
                           ref['depth'][slot].astype(f32), ref['rgb'][slot].astype(f32), go, gd, case['gr'][slot], gw, mutant=mutant)
    got.update(dsigma=tc.to_flat(ds.astype(np.float64), d['idx'], d['mask'], M), drgb=tc.to_flat(dr.astype(np.float64), d['idx'], d['mask'], M))
    return got


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('name', tc.CASES)
def test_case_conditions(name):
    case, ref = tc.cases()[name], tc.train_reference(name)
    N, stop = ref['N'], ref['stop']
    print(f'\n{name}: {len(N)} rows, {case["sigmas"].shape[0]} samples ({int(N.sum())} owned), threshold rays {int(ref["threshold"].sum())}, '
          f'rays that stop {int((stop >= 0).sum())}')
    assert ref['threshold'].sum() == 0
    assert len(N) == tc.N_RAYS and len(N) % 4 != 0
    assert all((N == length).sum() >= 3 for length in tc.LENGTHS)
    rays_a = case['rays_a']
    order = np.argsort(rays_a[:, 1])
    assert (order != np.arange(len(N))).any() and (rays_a[:, 0] != np.arange(len(N))).any() and (rays_a[:, 0] != np.argsort(order)).any()
    assert sorted(rays_a[:, 0]) == list(range(len(N)))
    first, length = rays_a[order, 1], rays_a[order, 2]
    gaps = first - np.concatenate([[0], (first + length)[:-1]])       # samples no ray owns, in front of every ray
    assert gaps.min() >= 1 and gaps.max() <= 70 and np.isnan(case['sigmas'][~(ref['owner'] >= 0)]).all()
    if name == 'stops':
        at = set(stop[stop >= 0].tolist())
        assert {0, 63, 64, 65} <= at and max(at) >= 128
        assert ((stop == N - 1) & (N > 0)).any()
        planned = sum(((N == length) & (stop == k)).any() for length, k in tc.STOP_PLAN)
        assert planned == len(tc.STOP_PLAN) and (stop >= 0).sum() > len(tc.STOP_PLAN)     # the constructed ones and rays dense enough to stop on their own
    if name == 'thr0':
        assert case['T_threshold'] == 0.0 and (stop < 0).all() and np.nanmax(case['sigmas'] * case['deltas']) <= 10
        np.testing.assert_array_equal(ref['total'][rays_a[:, 0]], N)
    if name == 'tie':
        assert case['T_threshold'] == 1.0 and (ref['total'] == 0).all() and (stop[N > 0] == 0).all()
        first = case['sigmas'][rays_a[N > 0, 1]]
        assert 0.2 < (first == 0).mean() < 0.5 and (ref['ws'][rays_a[N > 0, 1]][first == 0] == 0).all()
    if name == 'extremes':
        _, marks = tc.extremes(tc.SEEDS['extremes'])
        s = case['sigmas']
        assert np.isinf(s[~np.isnan(s)]).sum() == 5 and (s == f32(3e38)).sum() == 5 and all((s[r[1]:r[1] + r[2]] == 0).all() for r in rays_a[marks['zero']])
        assert (case['rgbs'] == f32(-0.25)).any() and (case['rgbs'] == f32(1.5)).any()
        assert (case['deltas'][np.isinf(s)] > 0).all()
        mag = np.abs(case['gr']).max(axis=1)
        assert mag.min() < 1e-5 and mag.max() > 1e2
        assert np.isfinite(ref['dsigma']).all()


# ------------------------------------------------------------------------------------------------ the emulation inside, the mutants outside
@pytest.mark.parametrize('name,null_grads', [(n, False) for n in tc.CASES] + [('extremes', True)])
def test_f32_emulation_stays_inside_every_budget(name, null_grads):
    ref, got = tc.train_reference(name, null_grads), _emulation(name, None, null_grads)
    worst = dict(tc.judge_train_fw(got, ref, name), **tc.judge_train_bw(got, ref, name))
    print(f'\n{name}{" (NULL gradients)" if null_grads else ""}: f32 emulation err / budget ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 0.6     # and not by a hair


# mutant -> (case, what must fail, the message it fails with)
MUTANTS = {'carry_reset': ('plain', 'fw', 'err/budget'), 'exclusive_prefix': ('plain', 'bw', 'dsigma'), 'strict_threshold': ('tie', 'fw', 'err/budget'),
           'stop_not_composited': ('stops', 'fw', 'err/budget'), 'count_includes_stop': ('stops', 'fw', 'total_samples'),
           'dws_sum_truncated': ('plain', 'bw', 'dsigma')}


@pytest.mark.parametrize('mutant', tuple(MUTANTS))
def test_wrong_kernels_fall_outside_the_budget(mutant):
    name, which, match = MUTANTS[mutant]
    ref, got = tc.train_reference(name), _emulation(name, mutant)
    with pytest.raises(AssertionError, match=match) as info:
        (tc.judge_train_fw if which == 'fw' else tc.judge_train_bw)(got, ref, f'{name} {mutant}')
    print(f'\n{mutant} on {name}: {str(info.value)[:200]}')
    if mutant == 'count_includes_stop':     # ... on the exact integer comparison: every float output of that mutant is inside its budget
        fixed = dict(got, total=ref['total'])
        tc.judge_train_fw(fixed, ref, name)
    if mutant == 'strict_threshold':      # the rays that open with sigma = 0 walk on into their second sample
        assert ((got['ws'] != 0) & ~ref['support']).sum() >= 10
    if mutant in ('carry_reset', 'exclusive_prefix'):      # by orders of magnitude, not by a hair
        key = 'ws' if mutant == 'carry_reset' else 'dsigma'
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.abs(got[key] - ref[key]) / ref['budget'][key]
        assert np.nanmax(np.where(np.isfinite(ratio), ratio, 0)) > 1e3


# ------------------------------------------------------------------------------------------------ the serial f32 C oracle inside the budgets
@pytest.mark.parametrize('name', ['plain', 'stops'])
def test_c_oracle_lies_inside_the_budgets(name):
    case, ref = tc.cases()[name], tc.train_reference(name)
    z = lambda v: np.nan_to_num(v, nan=0.0)       # samples no ray owns: the oracle forms dL_dws * ws over all of them
    args = [z(case[k]) for k in ('sigmas', 'rgbs', 'deltas', 'ts')]
    total, opacity, depth, rgb, ws = oracle.composite_train_fw(*args, case['rays_a'], case['T_threshold'])
    worst = tc.judge_train_fw(dict(total=total, opacity=opacity, depth=depth, rgb=rgb, ws=ws), ref, f'{name} oracle')
    r32 = lambda v: v.astype(f32)
    ds, dr = oracle.composite_train_bw(case['go'], case['gd'], case['gr'], case['gw'], args[0], args[1], r32(ref['ws']), args[2], args[3], case['rays_a'],
                                       r32(ref['opacity']), r32(ref['depth']), r32(ref['rgb']), case['T_threshold'])
    worst.update(tc.judge_train_bw(dict(dsigma=ds, drgb=dr), ref, f'{name} oracle'))
    print(f'\n{name}: C oracle err / budget ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('name', ['plain', 'stops'])
def test_c_oracle_distortion_lies_inside_the_budgets(name):
    c, ref = tc.distortion_cases()[name], tc.distortion_reference(name)
    z = lambda v: np.nan_to_num(v, nan=0.0)
    loss, wi, wti = oracle.distortion_loss_fw(c['ws'], z(c['deltas']), z(c['ts']), c['rays_a'])
    worst = _judge_distortion(dict(loss=loss, ws_incl=wi, wts_incl=wti), ref, f'{name} oracle')
    dws = oracle.distortion_loss_bw(c['g_loss'], ref['ws_incl'].astype(f32), ref['wts_incl'].astype(f32), c['ws'], z(c['deltas']), z(c['ts']), c['rays_a'])
    worst['dws'] = tc.assert_within_budget(dws, ref['dws'], ref['budget']['dws'], f'{name} oracle dws', owner=ref['owner'])
    print(f'\n{name}: C oracle distortion err / budget ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('n_samples', tc.INFERENCE_N)
def test_c_oracle_inference_lies_inside_the_budgets(n_samples):
    c, ref = tc.inference_case(n_samples), tc.inference_reference(n_samples)
    assert ref['threshold'].sum() == 0
    assert (ref['N'] == 0).any() and (ref['N'] == n_samples).any() and (ref['stop'] >= 0).any() and ((ref['stop'] < 0) & (ref['N'] > 0)).any()
    if n_samples > 64:
        assert (ref['stop'] == 64).any() and (ref['stop'] == n_samples - 1).any() and ((ref['stop'] >= 0) & (ref['stop'] < 64) & (ref['N'] > 64)).any()
    alive, op, dp, col = c['alive'].copy(), c['opacity'].copy(), c['depth'].copy(), c['rgb'].copy()
    oracle.composite_test_fw(c['sigmas'], c['rgbs'], c['deltas'], c['ts'], alive, c['T_threshold'], c['n_eff'], op, dp, col)
    worst = _judge_inference(dict(alive=alive, opacity=op, depth=dp, rgb=col), ref, f'inference {n_samples} oracle')
    # ... and the chunked f32 emulation, in the group width the kernel picks for this row length
    G = min(64, 1 << max(n_samples - 1, 0).bit_length())
    r = c['alive']
    emu = tc.emulate_fw(c['sigmas'], c['rgbs'], c['deltas'], c['ts'], c['n_eff'], c['T_threshold'], T0=f32(1) - c['opacity'][r], G=G)
    got = dict(alive=np.where((c['n_eff'] == 0) | emu['stopped'], -1, r))
    for key in ('opacity', 'depth', 'rgb'):
        v = c[key].copy()
        v[r] = np.where((c['n_eff'] > 0).reshape((-1,) + (1,) * (v.ndim - 1)), v[r] + emu[key], v[r])
        got[key] = v
    worst_e = _judge_inference(got, ref, f'inference {n_samples} emulation')
    print(f'\ninference {n_samples}: oracle {worst}, emulation (groups of {G}) {worst_e}')


def _judge_inference(got, ref, name):
    np.testing.assert_array_equal(got['alive'], ref['alive'], err_msg=f'{name}: alive')
    return {k: round(tc.assert_within_budget(got[k], ref[k], ref['budget'][k], f'{name} {k}'), 3) for k in ('opacity', 'depth', 'rgb')}


def _judge_distortion(got, ref, name):
    worst = {'loss': tc.assert_within_budget(got['loss'], ref['loss'], ref['budget']['loss'], f'{name} loss', rows=ref['row_of_slot'])}
    for k in ('ws_incl', 'wts_incl'):
        worst[k] = tc.assert_within_budget(got[k], ref[k], ref['budget'][k], f'{name} {k}', owner=ref['owner'])
    return worst


# ------------------------------------------------------------------------------------------------ distortion, march, fused: emulations
@pytest.mark.parametrize('name', ['plain', 'stops', 'equal_ts'])
def test_distortion_emulation_inside_and_its_mutant_outside(name):
    c, ref = tc.distortion_cases()[name], tc.distortion_reference(name)
    idx, mask = tc.dense_index(c['rays_a'], tc.K_MAX)
    slot, N, M = c['rays_a'][:, 0], c['rays_a'][:, 2], c['ws'].shape[0]
    w, dl, t = (tc.to_dense(c[k], idx, mask).astype(f32) for k in ('ws', 'deltas', 'ts'))
    if name == 'equal_ts':
        assert (np.diff(t, axis=1)[mask[:, 1:]] >= 0).all() and (np.diff(t, axis=1)[mask[:, 1:]] == 0).mean() > 0.5

    def run(mutant):
        loss, wi, wti = tc.emulate_distortion_fw(w, dl, t, N, mutant)
        by_slot = np.zeros(len(slot))
        by_slot[slot] = loss
        return dict(loss=by_slot, ws_incl=tc.to_flat(wi.astype(np.float64), idx, mask, M), wts_incl=tc.to_flat(wti.astype(np.float64), idx, mask, M))
    worst = _judge_distortion(run(None), ref, name)
    wi32, wti32 = (tc.to_dense(ref[k], idx, mask).astype(f32) for k in ('ws_incl', 'wts_incl'))
    dws = tc.emulate_distortion_bw(c['g_loss'][slot], wi32, wti32, w, dl, t, N)
    worst['dws'] = tc.assert_within_budget(tc.to_flat(dws.astype(np.float64), idx, mask, M), ref['dws'], ref['budget']['dws'], f'{name} dws', owner=ref['owner'])
    print(f'\ndistortion {name}: f32 emulation err / budget ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    with pytest.raises(AssertionError, match='err/budget'):
        _judge_distortion(run('distortion_carry_reset'), ref, f'{name} distortion_carry_reset')
    # the prefix form and the closed-form gradient are the definition and its autograd gradient
    scale = np.abs(tc.to_dense(ref['dws'], idx, mask)).max(axis=1)[ref['owner'][ref['owner'] >= 0]]
    own = ref['owner'] >= 0
    assert (np.abs(ref['closed_dws'] - ref['dws'])[own] <= 1e-10 * scale + 1e-300).all()
    # rays of length 0 and 1
    assert (ref['loss'][slot[N == 0]] == 0).all()
    one = np.nonzero(N == 1)[0]
    s0 = c['rays_a'][one, 1]
    np.testing.assert_allclose(ref['loss'][slot[one]], c['ws'][s0].astype(np.float64) ** 2 * c['deltas'][s0] / 3, rtol=1e-14)


@pytest.mark.parametrize('with_dirs', [True, False])
def test_march_backward_serial_f32_sums_inside_the_budget(with_dirs):
    c, ref = tc.march_case(), tc.march_reference(with_dirs)
    g_o, g_d = np.zeros((tc.N_RAYS, 3), f32), np.zeros((tc.N_RAYS, 3), f32)
    for n, (_, start, N) in enumerate(c['rays_a']):
        for s in range(start, start + N):
            g_o[n] += c['g_xyzs'][s]
            g_d[n] += c['g_xyzs'][s] * c['ts'][s]
            if with_dirs:
                g_d[n] += c['g_dirs'][s]
    worst = {k: tc.assert_within_budget(v, ref[k], ref['budget'][k], f'march {k}') for k, v in (('g_o', g_o), ('g_d', g_d))}
    print(f'\nmarch backward, g_dirs {with_dirs}: serial f32 err / budget {worst}')
    assert (ref['budget']['g_o'][ref['N'] == 0] == 0).all() and (ref['g_d'][ref['N'] == 0] == 0).all()
    wrong = g_d.copy()
    wrong[ref['N'] > 64] -= (c['g_xyzs'] * c['ts'][:, None])[c['rays_a'][ref['N'] > 64, 1] + 64]      # one sample dropped at the first seam
    with pytest.raises(AssertionError, match='err/budget'):
        tc.assert_within_budget(wrong, ref['g_d'], ref['budget']['g_d'], 'march g_d without a sample')


def test_fused_loss_emulation_inside_every_budget():
    """emulate_fw -> pixel -> squared error -> pixel gradient -> emulate_bw, all in f32, like the fused kernel chains them."""
    case, ref = tc.fused_case(), tc.fused_reference()
    assert ref['threshold'].sum() == 0 and case['counter'][0] < case['sample_capacity'] and case['ray_capacity'] == 45 and case['counter'][1] == 37
    d, v = _dense32(case)
    slot, M, n_live = d['ray_idx'], case['sigmas'].shape[0], case['n_live']
    fw = tc.emulate_fw(v['sigmas'], v['rgbs'], v['deltas'], v['ts'], d['N'], case['T_threshold'])
    bg, scale = np.asarray(case['bg'], f32), f32(case['scale'])
    O, D, RGB = fw['opacity'], fw['depth'], fw['rgb']
    pix = (RGB + ((f32(1) - O)[:, None] * bg)).astype(f32)
    live = slot < n_live
    diff = np.where(live[:, None], pix - case['target'][slot], f32(0)).astype(f32)
    n_el = f32(3 * n_live)
    sq = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2]).astype(f32)

    def by_slot(a):
        out = np.zeros(a.shape, np.float64)
        out[slot] = a
        return out
    tot = f32(0)
    for x in by_slot(sq).astype(f32):
        tot = f32(tot + x)
    mean = f32(tot / n_el)
    g = (f32(2) / n_el * diff * scale).astype(f32)
    gO = (f32(0) - (g[:, 0] * bg[0] + g[:, 1] * bg[1] + g[:, 2] * bg[2])).astype(f32)
    ds, dr = tc.emulate_bw(v['sigmas'], v['rgbs'], v['deltas'], v['ts'], d['N'], case['T_threshold'], fw['ws'], O, D, RGB, gO, None, g, None)
    got = dict(pixel=by_slot(pix), alpha=by_slot(O), depth=by_slot((D / (O + f32(1e-6))).astype(f32)), loss2=np.array([mean, f32(mean * scale)], np.float64),
               dsigma=tc.to_flat(ds.astype(np.float64), d['idx'], d['mask'], M), drgb=tc.to_flat(dr.astype(np.float64), d['idx'], d['mask'], M))
    worst = {k: tc.assert_within_budget(got[k], ref[k], ref['budget'][k], f'fused {k}', owner=ref['owner'] if k in ('dsigma', 'drgb') else None)
             for k in ('pixel', 'alpha', 'depth', 'loss2', 'dsigma', 'drgb')}
    print('\nfused loss: f32 emulation err / budget ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert (ref['dsigma'][ref['dead_samples']] == 0).all() and (ref['drgb'][ref['dead_samples']] == 0).all() and ref['dead_samples'].sum() > 100
    assert (np.abs(ref['closed_dsigma'] - ref['dsigma']) <= 1e-9 * np.abs(ref['dsigma']).max()).all()


# ------------------------------------------------------------------------------------------------ closed form against autograd, budget ceilings
@pytest.mark.parametrize('name', ['plain', 'stops', 'thr0', 'tie'])
def test_closed_form_gradients_agree_with_autograd(name):
    """1e-10 relative to the largest |delta| * (sum of the absolute operands of the closed form's bracket) of the ray: the closed form subtracts
    numbers of that size (1 - O with O = 1 - 2e-9 at a constructed stop), so that is the scale its own float64 rounding lives on."""
    case, ref = tc.cases()[name], tc.train_reference(name)
    idx, mask = tc.dense_index(case['rays_a'], tc.K_MAX)
    scale = tc.to_dense(ref['closed_operands'], idx, mask).max(axis=1)
    per_sample = tc.to_flat(np.broadcast_to(scale[:, None], mask.shape), idx, mask, case['sigmas'].shape[0])
    err = np.abs(ref['closed_dsigma'] - ref['dsigma'])
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(err == 0, 0.0, err / per_sample)
    print(f'\n{name}: closed form against autograd, dsigma {rel.max():.2e} of the bracket operands, '
          f'{(err / np.maximum(np.abs(ref["dsigma"]).max(), 1e-300)).max():.2e} of max |dsigma|')
    assert (rel <= 1e-10).all()
    np.testing.assert_allclose(ref['closed_drgb'], ref['drgb'], rtol=1e-10, atol=0)


def test_budget_ceilings_on_plain():
    """The largest budget per output relative to the ray's largest |value|: it comes from the reference alone, and may not grow past twice
    the recorded figure."""
    case, ref = tc.cases()['plain'], tc.train_reference('plain')
    idx, mask = tc.dense_index(case['rays_a'], tc.K_MAX)
    slot = case['rays_a'][:, 0]
    fig = {}
    for key in ('ws', 'dsigma', 'drgb'):
        v, b = tc.to_dense(ref[key], idx, mask), tc.to_dense(ref['budget'][key], idx, mask)
        v, b = (a.reshape(len(slot), -1) for a in (v, b))
        has = np.abs(v).max(axis=1) > 0
        fig[key] = float((b.max(axis=1)[has] / np.abs(v).max(axis=1)[has]).max())
    for key in ('opacity', 'depth', 'rgb'):
        v, b = np.abs(ref[key]).reshape(len(slot), -1).max(axis=1), ref['budget'][key].reshape(len(slot), -1).max(axis=1)
        fig[key] = float((b[v > 0] / v[v > 0]).max())
    print('\nplain: largest budget / largest |value| of the ray: ' + ', '.join(f'{k} {v:.2e}' for k, v in fig.items()))
    for key, v in fig.items():
        assert v <= 2 * tc.PLAIN_CEILINGS[key], (key, v)
    assert fig['dsigma'] <= 2e-4
