"""CPU: the reference of the visibility-masked Adam step (tests/sparse_adam_ref.py) against the project's C oracle and the published formula, the comparison
helper against planted errors, and everything of the feature that can be checked without a device: the export, the argument validation of
nrc_adam_step_rows_multi, and FusedAdam.step(visibility=...) / render_image_training refusing what they must before they modify anything."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from nerficg_amd import _lib
from tests import sparse_adam_ref as SR

BETAS, EPS, LR = (0.9, 0.99), 1e-15, 1e-2


def _problem(P=37, width=3, seed=0, steps_before=2):
    """A state after `steps_before` dense steps (non-trivial moments), a gradient and a 40 % mask."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(P, width)).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    everything = np.ones(P, bool)
    for s in range(1, steps_before + 1):
        p, m, v = SR.step_f32(p, rng.normal(size=p.shape).astype(np.float32), m, v, everything, s, LR, BETAS, EPS)
    g = (rng.normal(size=p.shape) * np.exp(rng.normal(size=p.shape) * 3)).astype(np.float32)
    mask = rng.random(P) < 0.4
    mask[0], mask[1] = True, False
    return p, g, m, v, mask, steps_before + 1


@pytest.mark.parametrize('weight_decay,adam_w_mode', [(0.0, False), (0.01, False), (0.01, True)])
def test_f32_reference_agrees_with_the_c_oracle_on_visible_rows(weight_decay, adam_w_mode):
    """With bias correction the float32 restatement and oracle.adam_step (oracle/adam_oracle.c, the arbiter of the dense step) agree on the visible rows within
    the tolerances of tests/test_gpu_adam_parity.py (p: rtol 1e-6, atol 1e-7; m: atol 1e-12; v: atol 1e-20).  Recorded on the build machine (x86-64, the
    oracle compiled without FMA contraction): they agree BIT FOR BIT in all three cases, which the test prints but does not require."""
    p, g, m, v, mask, step = _problem()
    got = SR.step_f32(p, g, m, v, mask, step, LR, BETAS, EPS, weight_decay, adam_w_mode)
    want = oracle.adam_step(p, g, m, v, step, LR, BETAS, EPS, weight_decay, adam_w_mode)
    want = tuple(w.reshape(p.shape) for w in want)
    bitwise = all(np.array_equal(a[mask].view(np.int32), b[mask].view(np.int32)) for a, b in zip(got, want))
    print(f'f32 reference vs oracle.adam_step on visible rows (wd={weight_decay}, adam_w={adam_w_mode}): bit for bit = {bitwise}')
    SR.compare((p, m, v), got, want, mask, what='reference vs oracle')


def test_f32_reference_without_bias_correction_agrees_with_the_published_formula():
    p, g, m, v, mask, step = _problem(seed=1)
    got = SR.step_f32(p, g, m, v, mask, step, LR, BETAS, EPS, bias_correction=False)
    want = SR.published_f64(p, g, m, v, mask, LR, BETAS, EPS)
    for name, a, e, b in zip('pmv', got, want, (p, m, v)):
        np.testing.assert_allclose(a[mask], e[mask], rtol=1e-6, atol=0, err_msg=name)
        assert np.array_equal(a[~mask].view(np.int32), b[~mask].view(np.int32)) and np.array_equal(e[~mask], b[~mask].astype(np.float64)), name
    with_bc = SR.step_f32(p, g, m, v, mask, step, LR, BETAS, EPS, bias_correction=True)
    assert not np.allclose(with_bc[0][mask], want[0][mask], rtol=1e-6, atol=0)     # the switch does something


def test_mask_kinds():
    assert SR.row_mask(np.array([0, 2, 255], np.uint8)).tolist() == [False, True, True]
    assert SR.row_mask(np.array([-3, 0, 7], np.int32)).tolist() == [False, False, True]
    assert SR.row_mask(np.array([True, False])).tolist() == [True, False]
    with pytest.raises(ValueError):
        SR.row_mask(np.array([1.0], np.float32))
    with pytest.raises(ValueError):
        SR.row_mask(np.array([1], np.uint8), kind=1)


def _planted(name, p, g, m, v, mask, step):
    kw = dict(step=step, lr=LR, betas=BETAS, eps=EPS, bias_correction=False)
    good = SR.step_f32(p, g, m, v, mask, **kw)
    if name == 'invisible row decayed':           # what the dense step does to a row with a zero gradient
        out = tuple(a.copy() for a in good)
        r = int(np.nonzero(~mask)[0][0])
        out[1][r] *= np.float32(BETAS[0]); out[2][r] *= np.float32(BETAS[1])
        return out
    if name == 'visible row skipped':
        out = tuple(a.copy() for a in good)
        r = int(np.nonzero(mask)[0][0])
        out[0][r], out[1][r], out[2][r] = p[r], m[r], v[r]
        return out
    if name == 'mask shifted by one row':
        return SR.step_f32(p, g, m, v, np.roll(mask, 1), **kw)
    if name == 'mask indexed per element':        # mask[i] instead of mask[i // width]
        P, w = p.shape
        elem = np.resize(mask, P * w)
        flat = [a.reshape(-1, 1) for a in (p, g, m, v)]
        return tuple(a.reshape(P, w) for a in SR.step_f32(*flat, elem, **kw))
    if name == 'bias correction applied':
        return SR.step_f32(p, g, m, v, mask, **{**kw, 'bias_correction': True})
    raise KeyError(name)


@pytest.mark.parametrize('name', ['invisible row decayed', 'visible row skipped', 'mask shifted by one row', 'mask indexed per element', 'bias correction applied'])
def test_compare_rejects_planted_errors(name):
    p, g, m, v, mask, step = _problem(seed=2)
    good = SR.step_f32(p, g, m, v, mask, step, LR, BETAS, EPS, bias_correction=False)
    SR.compare((p, m, v), good, good, mask)                                   # the helper accepts the right answer
    wrong = _planted(name, p, g, m, v, mask, step)
    with pytest.raises(AssertionError):
        SR.compare((p, m, v), wrong, good, mask, what=name)


# ------------------------------------------------------------------------------------------------ the library without a device
@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_symbol_is_exported_and_the_abi_version_stands(lib):
    assert 'nrc_adam_step_rows_multi' in _lib.parse_header() and hasattr(lib, 'nrc_adam_step_rows_multi')
    assert lib.nrc_abi_version() == _lib.header_abi_version() == 22


def test_argument_validation_without_gpu(lib):
    n = 2
    fake = (ctypes.c_void_p * n)(0x1000, 0x2000)      # never dereferenced on these paths
    arr = ctypes.cast(fake, ctypes.c_void_p)
    widths = lambda *w: ctypes.cast((ctypes.c_int32 * n)(*w), ctypes.c_void_p)
    ones = ctypes.cast((ctypes.c_float * n)(1.0, 1.0), ctypes.c_void_p)
    zeros = ctypes.cast((ctypes.c_float * n)(0.0, 1.0), ctypes.c_void_p)
    mask = ctypes.c_void_p(0x3000)
    tail = (0.9, 0.99, 1e-15, 0.0, 0, None)

    def call(n_tensors=n, params=arr, grads=arr, m=arr, v=arr, w=None, n_rows=0, visible=mask, kind=0, lrs=ones, bc1=ones, bc2=ones):
        return lib.nrc_adam_step_rows_multi(n_tensors, params, grads, m, v, widths(3, 45) if w is None else w, n_rows, visible, kind, lrs, bc1, bc2, *tail)

    assert call() == 0                                              # n_rows == 0: NRC_OK, nothing launched
    assert call(kind=1) == 0
    for bad in (dict(params=None), dict(grads=None), dict(m=None), dict(v=None), dict(w=ctypes.c_void_p(None)), dict(visible=None), dict(lrs=None),
                dict(bc1=None), dict(bc2=None), dict(n_tensors=0), dict(n_tensors=-1), dict(n_tensors=13), dict(w=widths(3, 0)), dict(w=widths(-1, 4)),
                dict(n_rows=-1), dict(kind=2), dict(kind=-1), dict(bc1=zeros)):
        assert call(**bad) == -1, bad
    null_tensor = ctypes.cast((ctypes.c_void_p * n)(0x1000, None), ctypes.c_void_p)
    assert call(params=null_tensor, n_rows=5) == -1                 # a null tensor pointer with rows to step
    assert call(n_rows=2 ** 62, w=widths(3, 45)) == -1              # n_rows * width does not fit


# ------------------------------------------------------------------------------------------------ FusedAdam.step(visibility=...) without a device
def _cpu_optimizer(capturable=False):
    from nerficg_amd.apex_optimizers import FusedAdam
    P = 6
    a, b = torch.nn.Parameter(torch.randn(P, 3)), torch.nn.Parameter(torch.randn(P, 1))
    opt = FusedAdam([{'params': [a], 'name': 'a'}, {'params': [b], 'name': 'b'}], lr=1e-2, capturable=capturable)
    a.grad, b.grad = torch.randn(P, 3), torch.randn(P, 1)
    return opt, (a, b), P


def _snapshot(opt, params):
    return ([p._version for p in params], [p.detach().clone() for p in params], [g.get('step') for g in opt.param_groups], len(opt.state))


def _assert_untouched(opt, params, snap):
    now = _snapshot(opt, params)
    assert now[0] == snap[0] and now[2] == snap[2] and now[3] == snap[3] == 0
    assert all(torch.equal(x, y) for x, y in zip(now[1], snap[1]))


@pytest.mark.parametrize('case', ['cpu tensors', 'float mask', 'wrong length', 'capturable', 'two-dimensional mask', 'not a tensor'])
def test_step_with_visibility_refuses_before_it_modifies_anything(case, lib):
    opt, params, P = _cpu_optimizer(capturable=case == 'capturable')
    vis = {'cpu tensors': torch.ones(P, dtype=torch.bool), 'float mask': torch.ones(P), 'wrong length': torch.ones(P + 1, dtype=torch.bool),
           'capturable': torch.ones(P, dtype=torch.bool), 'two-dimensional mask': torch.ones(P, 1, dtype=torch.bool), 'not a tensor': [True] * P}[case]
    snap = _snapshot(opt, params)
    with pytest.raises((RuntimeError, ValueError)) as e:
        opt.step(visibility=vis)
    expected = {'cpu tensors': 'CUDA', 'float mask': 'dtype', 'wrong length': 'CUDA|rows', 'capturable': 'capturable', 'two-dimensional mask': 'shape',
                'not a tensor': 'tensor'}[case]
    assert e.match(expected), str(e.value)
    _assert_untouched(opt, params, snap)


def test_step_with_visibility_and_no_gradients_is_a_silent_no_op(lib):
    opt, params, P = _cpu_optimizer()
    for p in params:
        p.grad = None
    snap = _snapshot(opt, params)
    opt.step(visibility=torch.ones(P + 3))       # stale mask of another length and dtype: not even looked at
    _assert_untouched(opt, params, snap)


def test_grad_scaler_scalars_are_refused(lib):
    opt, params, P = _cpu_optimizer()
    opt.grad_scale = torch.ones(1)
    snap = _snapshot(opt, params)
    with pytest.raises(RuntimeError, match='GradScaler'):
        opt.step(visibility=torch.ones(P, dtype=torch.bool))
    _assert_untouched(opt, params, snap)


# ------------------------------------------------------------------------------------------------ the model's switches without a device
def _cpu_model(P=8):
    from nerficg_amd.gaussian_splatting import Gaussians
    return Gaussians(torch.randn(P, 3), torch.randn(P, 3), torch.randn(P, 4), torch.randn(P, 1), torch.randn(P, 1, 3), torch.randn(P, 15, 3))


def test_training_setup_switches():
    from nerficg_amd.apex_optimizers import FusedAdam
    g = _cpu_model()
    g.training_setup()
    assert g.sparse_adam is False and all(grp['bias_correction'] is True for grp in g.optimizer.param_groups)
    g.training_setup(sparse_adam=True, bias_correction=False)
    assert g.sparse_adam is True and isinstance(g.optimizer, FusedAdam) and all(grp['bias_correction'] is False for grp in g.optimizer.param_groups)
    with pytest.raises(RuntimeError, match='sparse_adam'):
        g.optimizer_step()                      # no radii: a silent dense step would be a different optimizer
    with pytest.raises(RuntimeError, match='sparse_adam'):
        _cpu_model().training_setup(sparse_adam=True, optimizer_class=torch.optim.Adam)


def test_fused_rest_step_is_refused_on_a_sparse_adam_model():
    """Raised before the rasterizer is reached, so it can be checked here."""
    from nerficg_amd.gaussian_splatting import PerspectiveCamera, render_image_training
    g = _cpu_model()
    g.training_setup(sparse_adam=True)
    cam = PerspectiveCamera(32, 32, 40.0, 40.0)
    with pytest.raises(RuntimeError, match='fuse_rest_step=True on a model set up with sparse_adam'):
        render_image_training(g, cam, torch.eye(4), fuse_rest_step=True)
