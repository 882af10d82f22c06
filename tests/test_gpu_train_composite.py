"""GPU: the training compositor, the fused compositing + colour loss, the distortion loss, the inference compositor and the ray gradients of
the training march against the float64 statements of tests/train_composite_ref.py.  Every element of every output is judged by its own
first-order f32 budget, none exempt; integer outputs (total_samples, alive) and the support of ws and of the gradients must match exactly
(the cases hold no threshold rays).  Everything goes through the C ABI with raw pointers, or the thin wrappers / autograd classes of
nerficg_amd.VolumeRenderingV2; output buffers are pre-filled with a sentinel, so "zero where nobody writes" is tested, not assumed.

  a. nrc_composite_train_fw        ray lengths 0 .. 1024 with chunk seams at 63 / 64 / 65 / 128 / 129, stops on lane 0, lane 63, in later chunks
                                   and on a ray's last sample, T_threshold 0 and 1, sigma 0 / 3e38 / inf
  b. nrc_composite_train_bw        fed the float64 forward rounded to f32; NULL dL_dopacity / dL_ddepth / dL_dws; VolumeRenderer.apply end to end
  c. nrc_ngp_train_loss            pixel, alpha, depth, both losses, both gradients, the rows that are not live, the clearing ranges, the ticket
  d. nrc_distortion_loss_fw / _bw  and DistortionLoss.apply, with runs of equal ts
  e. nrc_composite_test_fw         rows of 1 .. 130 samples: every group width and the second trip of the chunk loop
  f. nrc_raymarching_train_bw      with and without dL_ddirs

Measured on MI355X, max |error| / budget per output (printed with -s):
    train fw        plain    opacity 0.324, depth 0.323, rgb 0.345, ws 0.485        stops  0.367, 0.367, 0.367, 0.498      thr0  0.344, 0.346, 0.375, 0.497
                    tie      0.397, 0.396, 0.397, 0.397                              extremes  0.257, 0.257, 0.254, 0.464
    train bw        plain    dsigma 0.072, drgb 0.485     stops 0.080, 0.498     thr0 0.098, 0.497     tie 0.122, 0.397     extremes 0.156, 0.464
                    extremes with NULL gradients 0.130, 0.464
    VolumeRenderer.apply, stops   opacity 0.367, depth 0.367, rgb 0.367, ws 0.498, dsigma 0.062, drgb 0.498
    fused loss      pixel 0.146, alpha 0.367, depth 0.114, loss2 0.001, dsigma 0.014, drgb 0.494
    distortion      plain    loss 0.172, ws_incl 0.388, wts_incl 0.358, dws 0.383, apply loss 0.172, apply dws 0.109
                    stops    0.111, 0.356, 0.391, 0.356, 0.111, 0.056        equal_ts  0.172, 0.388, 0.399, 0.389, 0.172, 0.137
    inference       rows of 1: opacity 0.285, depth 0.237, rgb 0.325    3: 0.322, 0.322, 0.317    8: 0.168, 0.220, 0.219    33: 0.186, 0.180, 0.295
                    64: 0.148, 0.145, 0.165    65: 0.088, 0.119, 0.211    130: 0.320, 0.318, 0.333
    march backward  g_o 0.373, g_d 0.357 (0.208 with dL_ddirs NULL)
No element over its budget, no integer output off: the tests exposed no defect in ngp_composite.hip.  (ws and drgb reach 0.5 where the CPU
emulation reaches 0.39: the emulation rounds a double-precision exponential once, the device's fast exponential uses part of the ulp that
EXP2_ULPS grants it.)
"""
import numpy as np
import pytest
import torch

from tests import train_composite_ref as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -7.0


def _T(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cases are read-only)


def _full(shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _lib_p():
    from nerficg_amd import _lib
    return _lib, _lib.load(), _lib.ptr


def _report(what, worst):
    print(f'\n{what}: err / budget ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ a. train forward
def _train_fw(case):
    _lib, lib, p = _lib_p()
    sig, rgbs, dl, ts, rays = (_T(case[k]) for k in ('sigmas', 'rgbs', 'deltas', 'ts', 'rays_a'))
    n, M = rays.shape[0], sig.shape[0]
    total, opacity, depth, rgb, ws = _full((n,), torch.int64), _full((n,)), _full((n,)), _full((n, 3)), _full((M,))
    _lib.check(lib.nrc_composite_train_fw(p(sig), p(rgbs), p(dl), p(ts), p(rays), n, M, float(case['T_threshold']), p(total), p(opacity), p(depth), p(rgb),
                                          p(ws), _lib.stream_of(sig)), 'composite_train_fw')
    torch.cuda.synchronize()
    return dict(total=total.cpu().numpy(), opacity=opacity.cpu().numpy(), depth=depth.cpu().numpy(), rgb=rgb.cpu().numpy(), ws=ws.cpu().numpy())


@pytest.mark.parametrize('name', tc.CASES)
def test_composite_train_fw(name):
    ref = tc.train_reference(name)
    got = _train_fw(tc.cases()[name])
    _report(f'train fw {name}', tc.judge_train_fw(got, ref, name))
    assert np.isfinite(got['ws']).all()


# ------------------------------------------------------------------------------------------------ b. train backward
def _train_bw(case, ref, null_grads=False):
    _lib, lib, p = _lib_p()
    sig, rgbs, dl, ts, rays = (_T(case[k]) for k in ('sigmas', 'rgbs', 'deltas', 'ts', 'rays_a'))
    n, M = rays.shape[0], sig.shape[0]
    ws, opacity, depth, rgb = (_T(ref[k].astype(np.float32)) for k in ('ws', 'opacity', 'depth', 'rgb'))
    go, gd, gr, gw = (_T(case[k]) for k in ('go', 'gd', 'gr', 'gw'))
    if null_grads:
        go = gd = gw = None
    ds, dr = _full((M,)), _full((M, 3))
    _lib.check(lib.nrc_composite_train_bw(p(go), p(gd), p(gr), p(gw), p(sig), p(rgbs), p(ws), p(dl), p(ts), p(rays), p(opacity), p(depth), p(rgb), n, M,
                                          float(case['T_threshold']), p(ds), p(dr), _lib.stream_of(sig)), 'composite_train_bw')
    torch.cuda.synchronize()
    return dict(dsigma=ds.cpu().numpy(), drgb=dr.cpu().numpy())


@pytest.mark.parametrize('name,null_grads', [(n, False) for n in tc.CASES] + [('extremes', True)])
def test_composite_train_bw(name, null_grads):
    ref = tc.train_reference(name, null_grads)
    got = _train_bw(tc.cases()[name], ref, null_grads)
    _report(f'train bw {name}{" (NULL gradients)" if null_grads else ""}', tc.judge_train_bw(got, ref, name))


def test_volume_renderer_apply_end_to_end_on_stops():
    """Forward and backward through the autograd class: the backward now gets the GPU's own f32 forward sums, not the rounded float64 ones --
    both are within one forward budget of the truth, so the same reference and a budget that charges the saved sums at their forward bound."""
    import nerficg_amd.VolumeRenderingV2 as vr
    case, ref = tc.cases()['stops'], tc.train_reference('stops')
    sig, rgbs = _T(case['sigmas']).requires_grad_(), _T(case['rgbs']).requires_grad_()
    n_comp, opacity, depth, rgb, ws = vr.VolumeRenderer.apply(sig, rgbs, _T(case['deltas']), _T(case['ts']), _T(case['rays_a']), case['T_threshold'])
    got = dict(total=ref['total'], opacity=opacity.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), rgb=rgb.detach().cpu().numpy(),
               ws=ws.detach().cpu().numpy())
    worst = tc.judge_train_fw(got, ref, 'apply stops')
    assert int(n_comp) == int(ref['total'].sum())
    (opacity * _T(case['go'])).sum().add((depth * _T(case['gd'])).sum()).add((rgb * _T(case['gr'])).sum()).add((ws * _T(case['gw'])).sum()).backward()
    budget = tc.train_reference_own_sums('stops')
    bw = dict(dsigma=sig.grad.cpu().numpy(), drgb=rgbs.grad.cpu().numpy())
    for k in ('dsigma', 'drgb'):
        worst[k] = tc.assert_within_budget(bw[k], ref[k], budget[k], f'apply stops {k}', owner=ref['owner'])
        assert (bw[k][~ref['support']] == 0).all()
    _report('VolumeRenderer.apply stops', worst)


# ------------------------------------------------------------------------------------------------ c. the fused loss
def test_fused_train_loss():
    _lib, lib, p = _lib_p()
    case, ref = tc.fused_case(), tc.fused_reference()
    cap_r, cap_s, M = case['ray_capacity'], case['sample_capacity'], case['sigmas'].shape[0]
    n_live, used = int(case['counter'][1]), int(case['counter'][0])

    def padded(a):
        out = np.full((cap_s,) + a.shape[1:], np.nan, np.float32)
        out[:M] = a
        return _T(out)
    sig, rgbs, dl, ts = (padded(case[k]) for k in ('sigmas', 'rgbs', 'deltas', 'ts'))
    rays, counter, target = _T(case['rays_a']), _T(case['counter']), _T(case['target'])
    bg, scale = _T(np.asarray(case['bg'], np.float32)), _T(np.asarray([case['scale']], np.float32))
    assert rays.shape[0] == cap_r and used < cap_s
    workspace = torch.zeros(int(lib.nrc_ngp_train_loss_ws_bytes(cap_r)), dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        ray_rgb, ray_alpha, ray_depth, loss2 = _full((cap_r, 3)), _full((cap_r,)), _full((cap_r,)), _full((2,))
        ds, dr, za, zb = _full((cap_s,)), _full((cap_s, 3)), _full((1000,)), _full((500,))
        _lib.check(lib.nrc_ngp_train_loss(p(sig), p(rgbs), p(dl), p(ts), p(rays), p(counter), cap_r, cap_s, float(case['T_threshold']), p(bg), p(target), p(scale),
                                          p(ray_rgb), p(ray_alpha), p(ray_depth), p(loss2), p(ds), p(dr), p(za[100:]), case['zero_a'], p(zb[50:]), case['zero_b'],
                                          p(workspace), _lib.stream_of(sig)), 'ngp_train_loss')
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in dict(pixel=ray_rgb, alpha=ray_alpha, depth=ray_depth, loss2=loss2, dsigma=ds, drgb=dr, za=za, zb=zb).items()})
        # the ticket words are back at zero (the per-ray partial sums behind them are not)
        assert int(workspace[:17 * 16 * 4].view(torch.int32).abs().sum()) == 0
    got = runs[0]
    for k, v in runs[1].items():
        np.testing.assert_array_equal(v, got[k], err_msg=f'second launch on the same workspace: {k}')
    worst = {k: tc.assert_within_budget(got[k], ref[k], ref['budget'][k], f'fused {k}', rows=ref['row_of_slot']) for k in ('pixel', 'alpha', 'depth')}
    worst['loss2'] = tc.assert_within_budget(got['loss2'], ref['loss2'], ref['budget']['loss2'], 'fused loss2')
    own = ref['owned']
    for k in ('dsigma', 'drgb'):
        g = got[k][:M]
        worst[k] = tc.assert_within_budget(g[own], ref[k][own], ref['budget'][k][own], f'fused {k}', owner=ref['owner'][own])
        assert (g[own & ~ref['support']] == 0).all(), f'{k}: not 0 behind a stop'
        assert (g[ref['dead_samples']] == 0).all(), f'{k}: not 0 in a row with ray_idx >= n_live'
        assert (got[k][used:] == 0).all(), f'{k}: not 0 at or beyond counter[0]'
    assert ref['dead_samples'].sum() > 100 and (np.sort(case['rays_a'][:, 0]) == np.arange(cap_r)).all() and n_live == 37
    # the two clearing ranges, and nothing around them
    for k, lo, n in (('za', 100, case['zero_a']), ('zb', 50, case['zero_b'])):
        assert (got[k][lo:lo + n] == 0).all() and (got[k][:lo] == SENTINEL).all() and (got[k][lo + n:] == SENTINEL).all(), k
    _report('fused loss', worst)


# ------------------------------------------------------------------------------------------------ d. the distortion loss
@pytest.mark.parametrize('name', ['plain', 'stops', 'equal_ts'])
def test_distortion_loss(name):
    _lib, lib, p = _lib_p()
    import nerficg_amd.VolumeRenderingV2 as vr
    c, ref = tc.distortion_cases()[name], tc.distortion_reference(name)
    ws, dl, ts, rays, g = (_T(c[k]) for k in ('ws', 'deltas', 'ts', 'rays_a', 'g_loss'))
    n, M = rays.shape[0], ws.shape[0]
    loss, wi, wti = _full((n,)), _full((M,)), _full((M,))
    _lib.check(lib.nrc_distortion_loss_fw(p(ws), p(dl), p(ts), p(rays), n, M, p(loss), p(wi), p(wti), _lib.stream_of(ws)), 'distortion_loss_fw')
    wi_in, wti_in = _T(ref['ws_incl'].astype(np.float32)), _T(ref['wts_incl'].astype(np.float32))
    dws = _full((M,))
    _lib.check(lib.nrc_distortion_loss_bw(p(g), p(wi_in), p(wti_in), p(ws), p(dl), p(ts), p(rays), n, M, p(dws), _lib.stream_of(ws)), 'distortion_loss_bw')
    torch.cuda.synchronize()
    loss, wi, wti, dws = (v.cpu().numpy() for v in (loss, wi, wti, dws))
    worst = {'loss': tc.assert_within_budget(loss, ref['loss'], ref['budget']['loss'], f'{name} loss', rows=ref['row_of_slot'])}
    for k, v in (('ws_incl', wi), ('wts_incl', wti), ('dws', dws)):
        worst[k] = tc.assert_within_budget(v, ref[k], ref['budget'][k], f'{name} {k}', owner=ref['owner'])
        assert (v[ref['owner'] < 0] == 0).all()
    # a ray of length 0 leaves loss 0; a ray of length 1 gives w^2 delta / 3
    slot, N = c['rays_a'][:, 0], c['rays_a'][:, 2]
    assert (N == 0).sum() >= 3 and (loss[slot[N == 0]] == 0).all()
    s0 = c['rays_a'][N == 1, 1]
    want = c['ws'][s0].astype(np.float64) ** 2 * c['deltas'][s0] / 3
    assert (N == 1).sum() >= 3 and (np.abs(loss[slot[N == 1]] - want) <= 4 * tc.SAFETY * tc.U * want).all()
    # the autograd class: its backward reads the scans the forward kernel wrote
    own = tc.distortion_reference(name, 'computed')
    w_t = _T(c['ws']).requires_grad_()
    out = vr.DistortionLoss.apply(w_t, dl, ts, rays)
    worst['apply loss'] = tc.assert_within_budget(out.detach().cpu().numpy(), ref['loss'], ref['budget']['loss'], f'{name} apply loss', rows=ref['row_of_slot'])
    (out * g).sum().backward()
    worst['apply dws'] = tc.assert_within_budget(w_t.grad.cpu().numpy(), own['dws'], own['budget']['dws'], f'{name} apply dws', owner=ref['owner'])
    _report(f'distortion {name}', worst)


# ------------------------------------------------------------------------------------------------ e. inference compositing
@pytest.mark.parametrize('n_samples', tc.INFERENCE_N)
def test_composite_test_fw(n_samples):
    _lib, lib, p = _lib_p()
    c, ref = tc.inference_case(n_samples), tc.inference_reference(n_samples)
    sig, rgbs, dl, ts, alive, n_eff, opacity, depth, rgb = (_T(c[k]) for k in ('sigmas', 'rgbs', 'deltas', 'ts', 'alive', 'n_eff', 'opacity', 'depth', 'rgb'))
    assert sig.shape == (alive.shape[0], n_samples) and int(alive.max()) < opacity.shape[0]
    _lib.check(lib.nrc_composite_test_fw(p(sig), p(rgbs), p(dl), p(ts), p(alive), alive.shape[0], n_samples, float(c['T_threshold']), p(n_eff), p(opacity), p(depth),
                                         p(rgb), _lib.stream_of(sig)), 'composite_test_fw')
    torch.cuda.synchronize()
    np.testing.assert_array_equal(alive.cpu().numpy(), ref['alive'])
    worst = {k: tc.assert_within_budget(v.cpu().numpy(), ref[k], ref['budget'][k], f'inference {n_samples} {k}') for k, v in (('opacity', opacity), ('depth', depth), ('rgb', rgb))}
    _report(f'inference, rows of {n_samples}', worst)


# ------------------------------------------------------------------------------------------------ f. ray gradients of the march
@pytest.mark.parametrize('with_dirs', [True, False])
def test_raymarching_train_bw(with_dirs):
    _lib, lib, p = _lib_p()
    c, ref = tc.march_case(), tc.march_reference(with_dirs)
    gx, gdirs, ts, rays = _T(c['g_xyzs']), (_T(c['g_dirs']) if with_dirs else None), _T(c['ts']), _T(c['rays_a'])
    n, M = rays.shape[0], ts.shape[0]
    g_o, g_d = _full((n, 3)), _full((n, 3))
    _lib.check(lib.nrc_raymarching_train_bw(p(gx), p(gdirs), p(ts), p(rays), n, M, p(g_o), p(g_d), _lib.stream_of(ts)), 'raymarching_train_bw')
    torch.cuda.synchronize()
    g_o, g_d = g_o.cpu().numpy(), g_d.cpu().numpy()
    worst = {'g_o': tc.assert_within_budget(g_o, ref['g_o'], ref['budget']['g_o'], 'march g_o'), 'g_d': tc.assert_within_budget(g_d, ref['g_d'], ref['budget']['g_d'], 'march g_d')}
    empty = ref['N'] == 0
    assert empty.sum() >= 3 and (g_o[empty] == 0).all() and (g_d[empty] == 0).all()
    _report(f'march backward, dL_ddirs {"given" if with_dirs else "NULL"}', worst)
