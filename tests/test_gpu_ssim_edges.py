"""GPU: the SSIM kernels (nerficg_amd/csrc/ssim.hip) against oracle/ssim_oracle.c where renders actually live -- exactly flat white and black,
near-constant grey, hard silhouettes, identical images, values outside [0, 1] -- at tile-edge shapes of the 32 x 32 tile, with more than
4096 workgroups in the fused photometric loss, and through the wrapper's side paths.  Every pixel of the map, of the three derivative maps and
of the gradient is held to its own first-order f32 error budget (tests/ssim_cases.py); tests/test_ssim_cases_cpu.py shows that budget rejects
wrong kernels.  Each test prints its largest err / budget (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import ssim_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MAPS = sc.OUTPUTS[1:]


def _t(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)   # a copy: the shared references are read-only


@functools.lru_cache(maxsize=None)
def _reference(name, shape):
    """Inputs, the oracle's outputs and the budgets: computed once per (builder, shape), shared, read-only."""
    seed = sc.case_seed(name)
    a, b = sc.BUILDERS[name](shape, seed)
    w = sc.upstream(shape, seed)
    m, d1, d2, d3 = oracle.ssim_forward(a, b)
    ref = dict(zip(sc.OUTPUTS, (m, d1, d2, d3)))
    ref['grad'] = oracle.ssim_backward(a, b, w, d1, d2, d3)
    for v in (a, b, w, *ref.values()):
        v.setflags(write=False)
    return a, b, w, ref, sc.ssim_budget(a, b, w)


def _forward_backward_within_budget(name, shape):
    from nerficg_amd.fused_ssim import _FusedSSIMMap
    a, b, w, ref, bud = _reference(name, shape)
    ta = _t(a).requires_grad_(True)
    smap = _FusedSSIMMap.apply(sc.C1, sc.C2, ta, _t(b), 'same', True)
    saved = smap.grad_fn.saved_tensors            # (img1, img2, dm_dmu1, dm_dsigma1_sq, dm_dsigma12)
    got = {'map': smap.detach().cpu().numpy(), **{k: saved[2 + i].cpu().numpy() for i, k in enumerate(MAPS)}}
    (smap * _t(w)).sum().backward()
    got['grad'] = ta.grad.cpu().numpy()
    ratios = {}
    for k in (*sc.OUTPUTS, 'grad'):
        assert np.isfinite(got[k]).all(), f'{name} {shape} {k}: not finite'
        ratios[k] = sc.assert_within_budget(got[k], ref[k], bud[k], f'{name} {shape} {k}')
    print(f'\nerr/budget {name} {shape}: ' + ' '.join(f'{k}={v:.3f}' for k, v in ratios.items()))
    if name == 'noise':   # common ground with test_gpu_ssim_parity.py: nowhere weaker than its absolute tolerances
        np.testing.assert_allclose(got['map'], ref['map'], rtol=0, atol=2e-6)
        np.testing.assert_allclose(got['grad'], ref['grad'], rtol=0, atol=2e-5 * np.abs(ref['grad']).max())
    return ratios


@pytest.mark.parametrize('name', list(sc.BUILDERS))
def test_content_map_derivative_maps_and_gradient_within_budget(name):
    _forward_backward_within_budget(name, sc.case_shape(name))


# H, W from {1, 5, 10, 11, 31, 32, 33, 42, 43, 64, 65}: the tile (32), the tile +- 1, the halo tile (42) +- 1, the window (11) and its radius
TILE_EDGES = [(32, 32), (33, 32), (32, 33), (64, 65), (65, 64), (1, 65), (65, 1), (1, 1), (11, 43), (5, 10), (10, 31), (31, 42), (42, 11),
              (43, 33), (33, 5), (64, 64), (65, 65)]


@pytest.mark.parametrize('hw', TILE_EDGES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
@pytest.mark.parametrize('name', ['noise', 'flat_white'])
def test_tile_edges_two_differing_planes(name, hw):
    _forward_backward_within_budget(name, (1, 2) + hw)


# ------------------------------------------------------------------------------------------------ the fused photometric loss
def _photometric_reference(a, b, l1w, dw, up):
    n = a.size
    m, d1, d2, d3 = oracle.ssim_forward(a, b)
    l1 = np.abs(a.astype(np.float64) - b).mean()
    ssim = m.astype(np.float64).mean()
    dl = np.full(a.shape, -dw * up / n, np.float32)
    grad = oracle.ssim_backward(a, b, dl, d1, d2, d3).astype(np.float64) + up * l1w / n * np.sign(a.astype(np.float64) - b)
    return l1w * l1 + dw * (1.0 - ssim), l1, ssim, grad, dl


def _run_photometric(a, b, l1w, dw, up):
    from nerficg_amd.fused_ssim import photometric_loss
    ta = _t(a).requires_grad_(True)
    val = photometric_loss(ta, _t(b), l1w, dw)
    terms = val.grad_fn.terms
    (val * torch.tensor(up, device=DEV)).backward()
    return val, terms.cpu().numpy(), ta.grad.cpu().numpy()


# planes * ceil(W / 32) * ceil(H / 32) workgroups: k_photo_reduce takes 4 * 1024 partials per trip of its loop
@pytest.mark.parametrize('shape, workgroups', [((65, 63, 3, 5), 4095), ((32, 64, 2, 33), 4096), ((241, 17, 3, 5), 4097), ((3, 2731, 3, 5), 8193)])
def test_photometric_loss_many_workgroups(shape, workgroups):
    """Value, ctx.terms and gradient around and beyond one trip of the reduction's loop, tolerances of
    test_photometric_loss_is_l1_plus_dssim_against_oracle_and_tensor_operations."""
    assert shape[0] * shape[1] * ((shape[3] + 31) // 32) * ((shape[2] + 31) // 32) == workgroups and shape[0] * shape[1] <= 65535
    a, b = sc.noise(shape, workgroups)
    a = a.copy()
    a[..., :1, :2] = b[..., :1, :2]        # exact ties: sign 0
    l1w, dw, up = 0.8, 0.2, 3.7
    ref_val, ref_l1, ref_ssim, ref_grad, _ = _photometric_reference(a, b, l1w, dw, up)
    val, terms, grad = _run_photometric(a, b, l1w, dw, up)
    print(f'\nphotometric {shape}: value err {abs(val.item() - ref_val):.2e} l1 err {abs(terms[1] - ref_l1):.2e} ssim err {abs(terms[2] - ref_ssim):.2e} '
          f'grad err / scale {np.abs(grad - ref_grad).max() / np.abs(ref_grad).max():.2e}')
    assert abs(val.item() - ref_val) < 3e-6
    assert terms[0] == val.item() and abs(terms[1] - ref_l1) < 3e-6 and abs(terms[2] - ref_ssim) < 3e-6
    np.testing.assert_allclose(grad, ref_grad, rtol=0, atol=2e-5 * np.abs(ref_grad).max())


def test_photometric_loss_flat_white_within_budget():
    """(1, 3, 33, 65) flat white.  The gradient's budget is the SSIM gradient's for dL_dmap = -lambda_dssim g / n, plus the roundings the fused
    node adds: the device product c_ssim * g against the oracle's f32 dL_dmap (3 u of every term), the L1 term c_l1 * g * sign (2 u) and its
    addition (u).  The sums: 4 + 6 + 2 f32 additions per workgroup (12 u of the sum of magnitudes, 13 u with the subtraction for L1), double
    after that, one f32 store."""
    shape = (1, 3, 33, 65)
    a, b = sc.flat_white(shape, sc.case_seed('flat_white'))
    l1w, dw, up = 0.8, 0.2, 3.7
    ref_val, ref_l1, ref_ssim, ref_grad, dl = _photometric_reference(a, b, l1w, dw, up)
    val, terms, grad = _run_photometric(a, b, l1w, dw, up)
    bud = sc.ssim_budget(a, b, dl)
    u, s = sc.U, sc.SAFETY
    l1_term = np.abs(up * l1w / a.size * np.sign(a.astype(np.float64) - b))
    grad_budget = bud['grad'] + s * u * (3 * bud['grad_terms'] + 3 * l1_term + np.abs(ref_grad))
    ratio = sc.assert_within_budget(grad, ref_grad, grad_budget, 'photometric flat_white grad')
    m = oracle.ssim_forward(a, b)[0].astype(np.float64)
    tol_ssim = bud['map'].mean() + s * u * (12 * np.abs(m).mean() + abs(ref_ssim))
    tol_l1 = s * u * 14 * ref_l1
    tol_val = l1w * tol_l1 + dw * tol_ssim + s * u * abs(ref_val)
    print(f'\nphotometric flat_white: grad err/budget {ratio:.3f}; value err {abs(val.item() - ref_val):.2e} (tol {tol_val:.2e}) '
          f'l1 err {abs(terms[1] - ref_l1):.2e} (tol {tol_l1:.2e}) ssim err {abs(terms[2] - ref_ssim):.2e} (tol {tol_ssim:.2e})')
    assert abs(val.item() - ref_val) <= tol_val
    assert abs(terms[1] - ref_l1) <= tol_l1 and abs(terms[2] - ref_ssim) <= tol_ssim
    assert np.isfinite(grad).all()


def test_photometric_loss_without_gradient_is_the_same_value_and_saves_nothing():
    """No gradient wanted: k_ssim_fwd<false, true>.  Same bits as the training-mode value, no graph, and no derivative maps allocated."""
    from nerficg_amd.fused_ssim import photometric_loss
    shape = (1, 3, 70, 100)
    a, b = sc.noise(shape, 11)
    ta, tb = _t(a), _t(b)
    train = photometric_loss(ta.clone().requires_grad_(True), tb, 0.8, 0.2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    val = photometric_loss(ta, tb, 0.8, 0.2)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(DEV) - before
    assert val.grad_fn is None and not val.requires_grad
    assert extra < a.nbytes, f'{extra} bytes allocated for a value-only call; one derivative map is {a.nbytes}'
    assert torch.equal(val, train.detach())
    m = oracle.ssim_forward(a, b)[0].astype(np.float64)
    assert abs(val.item() - (0.8 * np.abs(a.astype(np.float64) - b).mean() + 0.2 * (1.0 - m.mean()))) < 3e-6


# ------------------------------------------------------------------------------------------------ wrapper paths
def test_valid_padding_gradient_matches_oracle_with_zero_frame():
    from nerficg_amd.fused_ssim import _FusedSSIMMap
    shape = (1, 2, 33, 43)
    a, b = sc.noise(shape, 3)
    w = np.zeros(shape, np.float32)
    w[..., 5:-5, 5:-5] = sc.upstream(shape, 3)[..., 5:-5, 5:-5]
    ta = _t(a).requires_grad_(True)
    smap = _FusedSSIMMap.apply(sc.C1, sc.C2, ta, _t(b), 'valid', True)
    assert smap.shape == (1, 2, 23, 33)
    m, d1, d2, d3 = oracle.ssim_forward(a, b)
    bud = sc.ssim_budget(a, b, w)
    sc.assert_within_budget(smap.detach().cpu().numpy(), m[..., 5:-5, 5:-5], bud['map'][..., 5:-5, 5:-5], 'valid map')
    (smap * _t(w[..., 5:-5, 5:-5])).sum().backward()
    ref = oracle.ssim_backward(a, b, w, d1, d2, d3)
    ratio = sc.assert_within_budget(ta.grad.cpu().numpy(), ref, bud['grad'], 'valid grad')
    np.testing.assert_allclose(ta.grad.cpu().numpy(), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    print(f'\nvalid padding: grad err/budget {ratio:.3f}')


def test_backward_after_train_false_raises():
    from nerficg_amd.fused_ssim import _FusedSSIMMap, fused_ssim
    a, b = sc.noise((1, 1, 12, 12), 1)
    ta = _t(a).requires_grad_(True)
    smap = _FusedSSIMMap.apply(sc.C1, sc.C2, ta, _t(b), 'same', False)
    with pytest.raises(RuntimeError, match='train=True'):
        smap.sum().backward()
    tc = _t(a).requires_grad_(True)
    with pytest.raises(RuntimeError, match='train=True'):
        fused_ssim(tc, _t(b), train=False).backward()
    assert ta.grad is None and tc.grad is None


@pytest.mark.parametrize('layout', ['channels_last', 'sliced'])
def test_non_contiguous_image_fused_ssim_copies_photometric_loss_refuses(layout):
    from nerficg_amd.fused_ssim import fused_ssim, photometric_loss
    shape = (2, 3, 20, 37)
    a, b = sc.planes_differ(shape, 9)
    tb = _t(b)
    if layout == 'channels_last':
        nc = _t(a).to(memory_format=torch.channels_last)
    else:
        wide = torch.zeros(shape[:-1] + (2 * shape[-1],), device=DEV)
        wide[..., ::2] = _t(a)
        nc = wide[..., ::2]
    assert not nc.is_contiguous() and torch.equal(nc, _t(a))
    nc.requires_grad_(True)
    tc = _t(a).requires_grad_(True)
    v_nc, v_c = fused_ssim(nc, tb), fused_ssim(tc, tb)
    v_nc.backward()
    v_c.backward()
    assert torch.equal(v_nc, v_c) and torch.equal(nc.grad, tc.grad)
    m = oracle.ssim_forward(a, b)[0].astype(np.float64)
    assert abs(v_c.item() - m.mean()) < 2e-6
    with pytest.raises(RuntimeError, match='contiguous'):
        photometric_loss(nc.detach(), tb)
    with pytest.raises(RuntimeError, match='contiguous'):
        photometric_loss(tc.detach(), nc.detach())


def test_more_than_65535_planes_is_an_error_and_the_next_call_works():
    from nerficg_amd.fused_ssim import fused_ssim, photometric_loss
    big = torch.full((65536, 1, 2, 2), 0.5, device=DEV)
    with pytest.raises(RuntimeError, match='ssim_forward failed'):
        fused_ssim(big, big)
    with pytest.raises(RuntimeError, match='photometric_loss_forward failed'):
        photometric_loss(big, big)
    torch.cuda.synchronize()
    a, b = sc.noise((1, 2, 9, 13), 2)
    m = oracle.ssim_forward(a, b)[0].astype(np.float64)
    assert abs(fused_ssim(_t(a), _t(b), train=False).item() - m.mean()) < 2e-6
    ref = 0.8 * np.abs(a.astype(np.float64) - b).mean() + 0.2 * (1.0 - m.mean())
    assert abs(photometric_loss(_t(a), _t(b)).item() - ref) < 3e-6
    # the largest plane count that is allowed still runs
    most = torch.full((65535, 1, 2, 2), 0.5, device=DEV)
    assert abs(fused_ssim(most, most, train=False).item() - 1.0) < 1e-6


def test_f16_input_raises():
    from nerficg_amd.fused_ssim import fused_ssim, photometric_loss
    x = torch.rand(1, 3, 8, 8, device=DEV)
    for fn in (fused_ssim, photometric_loss):
        with pytest.raises(RuntimeError, match='dtype'):
            fn(x.half(), x.half())
        with pytest.raises(RuntimeError, match='dtype'):
            fn(x, x.half())
