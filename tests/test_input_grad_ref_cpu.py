"""CPU: the float64 restatement behind the input-gradient tests (tests/input_grad_ref.py) against the oracle and against central differences, and the
argument checks of the two C entry points (nrc_grid_backward_input, nrc_sh_identity_backward_input), which run before any launch -- no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from nerficg_amd import _lib
from tests import input_grad_ref as R

GRID, SH = 'nrc_grid_backward_input', 'nrc_sh_identity_backward_input'


@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('n_levels,n_features,log2_t', [(16, 2, 19), (8, 4, 19), (16, 2, 14), (8, 4, 14)])
def test_restated_forward_equals_the_oracle_within_one_fp16_rounding(n_levels, n_features, log2_t):
    """Ties the restatement's cell, corner order, dense index and hash rule to oracle.grid_encode_fw (oracle_grid_encode_fwF): the float64 features,
    rounded by nobody, lie within one fp16 ulp of the oracle's fp16-rounded f32 ones, on every element -- faces and cell corners included."""
    cfg = R.grid_cfg(n_levels, n_features, log2_t)
    table = R.random_table(cfg, seed=1)
    x = R.positions(600, seed=2)
    mine = R.grid_forward(x, table, cfg)
    ref = oracle.grid_encode_fw(x, table, n_levels, log2_t, cfg['base_resolution'], cfg['per_level_scale'])
    ulp = np.maximum(2.0 ** -10 * np.abs(ref), 2.0 ** -24)
    assert mine.shape == ref.shape == (600, n_levels * n_features)
    assert np.all(np.abs(mine - ref) <= ulp), float(np.max(np.abs(mine - ref) / ulp))
    assert np.abs(ref).max() > 0.1


@pytest.mark.parametrize('n_levels,n_features,log2_t', [(16, 2, 19), (8, 4, 14), (5, 4, 19)])
def test_restated_derivative_equals_central_differences_of_its_forward(n_levels, n_features, log2_t):
    """At positions whose +-h neighbours stay inside the cell on every level and axis the interpolant is trilinear: the central difference of the float64
    forward, contracted with the upstream gradient, is the derivative up to float64 rounding.  Relative 1e-6 of the sum of |addends| of the element."""
    cfg = R.grid_cfg(n_levels, n_features, log2_t)
    table = R.random_table(cfg, seed=3)
    x = R.positions(400, seed=4)[len(R.SPECIAL_POSITIONS):]
    g = R.upstream(x.shape[0], n_levels * n_features, seed=5)
    h = 2.0 ** -24
    _, _, scales, _ = R._layout(cfg)
    interior = np.ones(x.shape[0], bool)
    for s in scales:
        _, frac = R._cells(x, s)
        interior &= np.all(np.minimum(frac, 1.0 - frac) > 2.0 ** -8, axis=1)   # scale h <= 2^-13
    assert interior.sum() >= 100
    x, g = x[interior], g[interior]
    grad, mag = R.grid_input_grad(x, g, table, cfg)
    g64 = g.astype(np.float64)
    for axis in range(3):
        step = np.zeros(3)
        step[axis] = h
        hi = (R.grid_forward(x, table, cfg, shift=step) * g64).sum(1)
        lo = (R.grid_forward(x, table, cfg, shift=-step) * g64).sum(1)
        fd = (hi - lo) / (2 * h)
        assert np.all(np.abs(fd - grad[:, axis]) <= 1e-6 * mag[:, axis] + 1e-300), float(np.max(np.abs(fd - grad[:, axis]) / (mag[:, axis] + 1e-300)))
    live = np.abs(g).sum(1) > 0
    assert np.all(grad[~live] == 0) and np.all(mag[~live] == 0) and np.all(np.abs(grad[live]).sum(1) > 0)
    assert np.all(np.abs(grad) <= mag)


def test_restated_sh_is_the_oracles_and_its_derivative_equals_central_differences():
    rng = np.random.default_rng(6)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d01 = (d * 0.5 + 0.5).astype(np.float16).astype(np.float64)
    sh = R.sh4_torch(torch.tensor(d01)).numpy()
    ref = oracle.sh4_encode(d01.astype(np.float32))
    assert np.all(np.abs(sh - ref) <= np.maximum(2.0 ** -10 * np.abs(ref), 2.0 ** -24) + 4 * R.U)   # fp16-rounded f32 polynomials
    g = R.upstream(300, 16, seed=7)
    grad, mag = R.sh_input_grad(d01, g)
    h = 2.0 ** -20
    for axis in range(3):
        step = np.zeros(3)
        step[axis] = h
        hi = (R.sh4_torch(torch.tensor(d01 + step)).numpy() * g).sum(1)
        lo = (R.sh4_torch(torch.tensor(d01 - step)).numpy() * g).sum(1)
        fd = (hi - lo) / (2 * h)   # cubic polynomials: the central difference is off by h^2 f''' / 6 ~ 1e-11 relative
        assert np.all(np.abs(fd - grad[:, axis]) <= 1e-6 * mag[:, axis] + 1e-300)
    assert np.all(np.abs(grad) <= mag * (1 + 1e-12))
    assert np.all(grad[1::4] == 0) and np.all(mag[1::4] == 0)
    # degree 1 is a constant: a gradient that lives on coefficient 0 alone gives no direction gradient
    g0 = np.zeros((300, 16), np.float32)
    g0[:, 0] = 1.0
    assert np.all(R.sh_input_grad(d01, g0)[0] == 0)


def test_header_declares_and_library_exports_both_entry_points(lib):
    protos = _lib.parse_header()
    assert _lib.header_abi_version() == lib.nrc_abi_version() >= 13
    ret, args = protos[GRID]
    assert ret == 'int'
    assert [a for _, a in args] == ['x01', 'M', 'd_features', 'd_features_pair_major', 'table_f16', 'n_levels', 'n_features', 'log2_hashmap_size',
                                    'base_resolution', 'per_level_scale', 'd_x01', 'stream']
    assert [t for t, _ in args] == ['const float*', 'int64_t', 'const float*', 'int32_t', 'const void*', 'int32_t', 'int32_t', 'int32_t', 'int32_t', 'float',
                                    'float*', 'nrc_stream_t']
    ret, args = protos[SH]
    assert ret == 'int'
    assert [a for _, a in args] == ['input_f16', 'input_ld', 'M', 'd_in', 'd_input', 'stream']
    assert [t for t, _ in args] == ['const void*', 'int32_t', 'int64_t', 'const float*', 'float*', 'nrc_stream_t']
    assert hasattr(lib, GRID) and hasattr(lib, SH)


def _host(n_bytes=4096):
    """a host buffer standing in for a device pointer: the calls below are refused before anything is launched or read"""
    buf = ctypes.create_string_buffer(n_bytes)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _grid_call(lib, **over):
    keep, p = _host()
    args = dict(x01=p, M=4, d_features=p, d_features_pair_major=0, table_f16=p, n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16,
                per_level_scale=R.PLS, d_x01=p, stream=None)
    assert list(args) == [a for _, a in _lib.parse_header()[GRID][1]]
    args.update(over)
    return getattr(lib, GRID)(*args.values())


@pytest.mark.parametrize('over', [dict(x01=None), dict(d_features=None), dict(table_f16=None), dict(d_x01=None), dict(M=-1),
                                  dict(n_features=1), dict(n_features=3), dict(n_features=8), dict(n_levels=0), dict(n_levels=17),
                                  dict(n_levels=16, n_features=4), dict(n_levels=9, n_features=4),
                                  dict(n_levels=8, n_features=4, d_features_pair_major=1), dict(d_features_pair_major=2),
                                  dict(per_level_scale=0.0), dict(log2_hashmap_size=0)])
def test_grid_entry_point_refuses_bad_arguments_before_any_launch(lib, over):
    assert _grid_call(lib, **over) == -1   # NRC_ERR_INVALID


def test_grid_entry_point_accepts_an_empty_batch_without_a_gpu(lib):
    assert _grid_call(lib, M=0) == 0
    assert _grid_call(lib, M=0, n_levels=8, n_features=4) == 0
    assert _grid_call(lib, M=0, x01=None, d_features=None, d_x01=None) == 0


@pytest.mark.parametrize('over', [dict(input_f16=None), dict(d_in=None), dict(d_input=None), dict(M=-1), dict(input_ld=18), dict(input_ld=0)])
def test_sh_entry_point_refuses_bad_arguments_before_any_launch(lib, over):
    keep, p = _host()
    args = dict(input_f16=p, input_ld=19, M=4, d_in=p, d_input=p, stream=None)
    assert list(args) == [a for _, a in _lib.parse_header()[SH][1]]
    args.update(over)
    assert getattr(lib, SH)(*args.values()) == -1
    assert getattr(lib, SH)(p, 19, 0, p, p, None) == 0
