"""CPU: the float64 restatement of the map losses (tests/map_losses_ref.py) against the reference's own functions (tests/golden/map_losses.npz, written by
tests/golden/make_map_losses_golden.py), the module's tensor formula against the restatement, the error budget against plain f32, and the new entry
points' host validation (include/nerficg_hip.h group 15)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import map_losses_ref as ref

GOLDEN = np.load(ref.__file__.replace('map_losses_ref.py', 'golden/map_losses.npz'))


def _close(got, want, what):
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-12, atol=1e-12 * max(float(np.abs(want).max()), 1e-300), err_msg=what)


@pytest.mark.parametrize('shape', ref.SHAPES)
def test_the_generator_reproduces_the_stored_inputs_with_the_margin(shape):
    key = 'x'.join(map(str, shape))
    depth, alpha, image = ref.inputs(shape)
    for name, t in (('depth', depth), ('alpha', alpha), ('image', image)):
        assert t.dtype == np.float32 and np.array_equal(t, GOLDEN[f'{key}_{name}']), name
    lap, dimg = ref.margins(depth, alpha, image)
    assert lap >= ref.MARGIN and dimg >= ref.MARGIN
    assert 0.05 <= alpha.min() and alpha.max() <= 0.95 and image.min() >= 0 and image.max() <= 1


@pytest.mark.parametrize('normalize,symmetrical', ref.GOLDEN_CONFIGS)
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_restatement_matches_the_reference_functions_in_float64(shape, normalize, symmetrical):
    key0, key = 'x'.join(map(str, shape)), ref.golden_key(shape, normalize, symmetrical)
    val = ref.evaluate(GOLDEN[key0 + '_depth'], GOLDEN[key0 + '_alpha'], GOLDEN[key0 + '_image'], ref.LAMBDA_SMOOTH, ref.LAMBDA_ENTROPY, normalize, symmetrical)
    _close(val['loss'], GOLDEN[key + '_loss'], 'loss')
    _close(val['S_x'] + val['S_y'], GOLDEN[key + '_S'], 'S_x + S_y')
    _close(val['E'], GOLDEN[key + '_E'], 'E')
    for name in ('g_depth', 'g_alpha', 'g_image'):
        _close(val[name], GOLDEN[key + '_' + name], name)


def _torch_formula(shape, normalize, symmetrical, weights, dtype):
    from nerficg_amd.map_losses import map_regularizer
    d, a, i = (torch.from_numpy(t).to(dtype).requires_grad_(True) for t in ref.inputs(shape))
    loss = map_regularizer(d, a, i, ref.f32(weights[0]), ref.f32(weights[1]), normalize=normalize, symmetrical=symmetrical)
    loss.backward()
    zero = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()
    return loss.item(), zero(d), zero(a), zero(i)


@pytest.mark.parametrize('name,shape,normalize,symmetrical,weights', [c for c in ref.all_cases() if c[1] not in (ref.MANY_WORKGROUPS, 'ties')])
def test_module_cpu_fallback_is_the_restatement(name, shape, normalize, symmetrical, weights):
    """float64 CPU tensors take the tensor formula.  (Not on `ties`: in float64 torch clamps at the doubles 1e-6 and 1 - 1e-6, the restatement at their f32
    values like the kernel and like torch in f32 -- the f32 test below covers the ties.)"""
    val, _ = ref.reference(shape, normalize, symmetrical, weights)
    loss, gd, ga, gi = _torch_formula(shape, normalize, symmetrical, weights, torch.float64)
    _close(loss, val['loss'], 'loss')
    for got, key in ((gd, 'g_depth'), (ga, 'g_alpha'), (gi, 'g_image')):
        _close(got, val[key], key)


def test_reference_signatures_on_cpu():
    from nerficg_amd.map_losses import background_entropy, depth_smoothness_loss
    depth, alpha, image = (torch.from_numpy(t.astype(np.float64)) for t in ref.inputs((2, 4, 33, 65)))
    val = ref.evaluate(depth.numpy(), alpha.numpy(), image.numpy(), 1.0, 1.0, False, True)
    _close(depth_smoothness_loss(depth[:, None], image).item(), val['S_x'] + val['S_y'], 'depth_smoothness_loss')
    _close(background_entropy(alpha, symmetrical=True).item(), val['E'], 'background_entropy')
    _close(background_entropy(alpha.reshape(-1)).item(), ref.evaluate(depth.numpy(), alpha.numpy(), image.numpy(), 0.0, 1.0, False, False)['E'], 'flat entropy')


@pytest.mark.parametrize('name,shape,normalize,symmetrical,weights', ref.all_cases())
def test_plain_f32_tensor_operations_stay_within_the_budget(name, shape, normalize, symmetrical, weights):
    """The tensor formula (nerficg_amd.map_losses.tensor_formula: the reference's functions in this project's words) as torch evaluates it in float32 passes the
    budget the kernels are held to, on every case, ties included: nothing but f32 rounding is needed to pass it."""
    val, bud = ref.reference(shape, normalize, symmetrical, weights)
    if shape != 'ties':
        lap, dimg = ref.margins(*ref.inputs(shape))
        assert lap >= ref.MARGIN and dimg >= ref.MARGIN
    loss, gd, ga, gi = _torch_formula(shape, normalize, symmetrical, weights, torch.float32)
    worst = {'loss': ref.assert_within_budget(loss, val['loss'], bud['loss'], 'loss')}
    for got, key in ((gd, 'g_depth'), (ga, 'g_alpha'), (gi, 'g_image')):
        worst[key] = ref.assert_within_budget(got, val[key], bud[key], key)
    print(name, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize('normalize,symmetrical', ref.GOLDEN_CONFIGS)
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_the_reference_functions_in_float32_stay_within_the_budget(shape, normalize, symmetrical):
    """The reference's OWN functions, evaluated by torch in float32 when the fixture was written, against the float64 restatement and the kernels' budget."""
    key = ref.golden_key(shape, normalize, symmetrical) + '_f32'
    val, bud = ref.reference(shape, normalize, symmetrical, ref.WEIGHTS[2])
    worst = {'loss': ref.assert_within_budget(GOLDEN[key + '_loss'], val['loss'], bud['loss'], 'loss')}
    for name in ('g_depth', 'g_alpha', 'g_image'):
        assert GOLDEN[key + '_' + name].dtype == np.float32
        worst[name] = ref.assert_within_budget(GOLDEN[key + '_' + name], val[name], bud[name], name)
    print(key, {k: round(v, 3) for k, v in worst.items()})


def test_ties_are_exact_zeros_in_the_restatement():
    depth, alpha, image = ref.ties()
    val = ref.evaluate(depth, alpha, image, 1.0, 1.0, False, False)
    d32, d64 = depth[0], depth[0].astype(np.float64)
    for lap in (d32[1:5, 1:3] + d32[1:5, 3:5] - 2 * d32[1:5, 2:4], d64[1:5, 1:3] + d64[1:5, 3:5] - 2 * d64[1:5, 2:4],          # centres x = 2, 3 of the patch
                d32[1:3, 1:5] + d32[3:5, 1:5] - 2 * d32[2:4, 1:5], d64[1:3, 1:5] + d64[3:5, 1:5] - 2 * d64[2:4, 1:5]):         # centres y = 2, 3
        assert not lap.any()                                           # f32 and f64 agree on the zero: sign(lap) = 0, the term has no gradient
    assert val['g_alpha'][0, 0, 0] == 0 and val['g_alpha'][0, 0, 1] == 0 and val['g_alpha'][0, 5, 6] == 0 and val['g_alpha'][0, 5, 5] == 0   # outside the clamp
    assert val['g_alpha'][0, 0, 2] != 0 and val['g_alpha'][0, 0, 3] != 0 and val['g_alpha'][0, 0, 4] != 0                                      # at the bounds, at 0.5
    assert (np.diff(image[0, :, 2:4, 2:5], axis=2) == 0).all()


def test_budget_maxima_on_the_named_case():
    got = ref.budget_maxima()
    print({k: f'{v:.3e}' for k, v in got.items()})
    for k, ceiling in ref.NAMED_CEILINGS.items():
        assert got[k] <= ceiling, (k, got[k])


def test_entry_points_validate_before_any_hip_call():
    from nerficg_amd import _lib
    lib = _lib.load()
    assert lib.nrc_abi_version() >= 9 and _lib.header_abi_version() >= 9
    buf = (ctypes.c_float * 64)()                                      # host memory standing in for device pointers: a refused call dereferences nothing
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda depth=p, alpha=p, image=p, B=1, C=3, H=8, W=8, ls=0.1, le=0.01, ws=p, out=p: lib.nrc_map_losses_forward(depth, alpha, image, B, C, H, W, 1, ls, le, 0, ws, out, None)
    bwd = lambda depth=p, alpha=p, image=p, B=1, C=3, H=8, W=8, ls=0.1, le=0.01, gd=p, ga=p, gi=p: lib.nrc_map_losses_backward(depth, alpha, image, B, C, H, W, 1, ls, le, 0, None, gd, ga, gi, None)
    for fn in (fwd, bwd):
        assert fn(depth=None) == -1 and fn(alpha=None) == -1 and fn(image=None) == -1
        assert fn(C=5) == -1 and fn(C=0) == -1 and fn(H=2) == -1 and fn(W=2) == -1 and fn(B=0) == -1
        assert fn(ls=0.0, le=0.0) == -1
    assert fwd(ws=None) == -1 and fwd(out=None) == -1
    assert bwd(gd=None, ga=None, gi=None) == -1 and bwd(ls=0.0, ga=None) == -1
    assert lib.nrc_map_losses_ws_floats(1, 2, 8) == -1 and lib.nrc_map_losses_ws_floats(0, 8, 8) == -1
    assert lib.nrc_map_losses_ws_floats(2, 33, 65) == 4 * 2 * 3 * 3 + 4
