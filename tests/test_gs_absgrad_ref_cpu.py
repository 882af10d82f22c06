"""CPU: the float64 reference of the absolute screen-space gradients (tests/gs_absgrad_ref.py) before it judges the kernel, and the C ABI of group 23.

  1. an independent statement: a float64 torch blend of the oracle's forward state (active sets as constants, alpha passing its gradient straight through the
     0.99 clamp), s_p = <g_p, C_p> per pixel (with the maps plus the depth and alpha terms), its Jacobian with respect to points_xy by autograd, times
     (W/2, H/2), |.| per pixel, summed over pixels: agrees with want_abs within 1e-10 A_q (both sides are float64 with a few hundred roundings, gamma_64 ~ 1e-13);
  2. properties: |S_q| <= want_abs <= A_q, want_abs(g) == want_abs(-g) exactly, want_abs == |S_q| exactly when one pixel carries the gradient, zero rows
     exactly where A == 0;
  3. the test can tell: with a +-1 checkerboard on all channels at least half of the live elements have want_abs - |S| > 100 B;
  4. planted errors: the judge rejects |signed sum|, abs after the per-(tile, 4 x 4 block) sum, abs after the per-tile sum, missing W/2, H/2 factors and x / y
     swapped, each in at least one Gaussian, on the case's own gradients and on the checkerboard;
  5. the entry point is declared and exported, its last arguments are the new output and the stream, the version is 22, and a bad band and a misaligned
     grad_records are refused through the C ABI without a device."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerficg_amd import _lib
from tests import gs_absgrad_ref as AR
from tests import gs_grad_cases as C
from tests import gs_grad_ref as R

NRC_OK, NRC_ERR_INVALID = 0, -1


def checkerboard(c):
    """(g, g_d, g_a): +-1 by the parity of x + y on every channel."""
    y, x = np.meshgrid(np.arange(c.h), np.arange(c.w), indexing='ij')
    s = np.where((x + y) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return np.stack([s, s, s]), s.copy(), s.copy()


EXTRA = {
    'partial-9x5-aux': lambda: C._case('partial-9x5-aux', w=9, h=5, aux='all'),
    'clamp-alpha-0.999-16x16': lambda: C._case('clamp-alpha-0.999-16x16', C._opaque_third(), w=16, h=16),
}


@functools.lru_cache(maxsize=None)
def _built(name, kind='own'):
    """(case, reference of gs_grad_cases, want_abs, budget, A): computed once, never modified."""
    c = C.get(name) if name in C.CASES else EXTRA[name]()
    st, _ = C.forward(c)
    r = C.reference(c, st, grads=None if kind == 'own' else checkerboard(c))
    args = (r.g, r.g_d, r.g_a) if c.aux else (r.g,)
    return c, r, AR.want_abs(r.blend, *args), AR.budget(r.B), AR.magnitude(r.ref)


def _args(c, r):
    return (r.g, r.g_d, r.g_a) if c.aux else (r.g,)


# ---------------------------------------------------------------------------------------------------- 1. the independent statement
def _torch_abs(c, r):
    """(P, 2): sum over pixels of |d s_p / d points_xy| (W/2, H/2), s_p the pixel's share of the loss, by float64 autograd, tile by tile."""
    f = torch.float64
    st = r.st64
    pts = torch.tensor(np.asarray(st.points_xy, np.float64), requires_grad=True)
    co, rgb, z = (torch.tensor(np.asarray(a, np.float64)) for a in (st.conic_opacity, st.rgb, st.depths))
    bg = torch.tensor(np.asarray(c.bg, np.float64))
    out = torch.zeros(st.P, 2, dtype=f)
    cap = torch.tensor(R.ALPHA_CAP, dtype=f)
    for tl in r.blend.tiles:
        ids = torch.tensor(tl.ids.astype(np.int64))
        px, py = torch.tensor(tl.px.astype(np.float64)), torch.tensor(tl.py.astype(np.float64))
        act = torch.tensor(tl.active)                                          # (K, N): a constant
        dx, dy = pts[ids, 0, None] - px[None, :], pts[ids, 1, None] - py[None, :]
        A, B, Cc, o = (co[ids, j, None] for j in range(4))
        oG = o * torch.exp(-0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy)
        alpha = oG + (torch.minimum(cap, oG) - oG).detach()                    # the clamp passes the gradient straight through
        alpha = torch.where(act, alpha, torch.zeros_like(alpha))
        T_in = torch.cumprod(torch.cat([torch.ones(1, alpha.shape[1], dtype=f), 1.0 - alpha], 0), 0)   # (K + 1, N): T in front of entry k; last row T_final
        w = alpha * T_in[:-1]
        g = [torch.tensor(r.g[ch][tl.py, tl.px].astype(np.float64)) for ch in range(3)]
        s = sum(g[ch] * ((w * rgb[ids, ch, None]).sum(0) + T_in[-1] * bg[ch]) for ch in range(3))
        if c.aux:
            s = s + torch.tensor(r.g_d[tl.py, tl.px].astype(np.float64)) * (w * z[ids, None]).sum(0) + torch.tensor(r.g_a[tl.py, tl.px].astype(np.float64)) * w.sum(0)
        for p in range(s.shape[0]):
            (jac,) = torch.autograd.grad(s[p], pts, retain_graph=True)
            out += jac.abs() * torch.tensor([0.5 * c.w, 0.5 * c.h], dtype=f)
    return out.numpy()


@pytest.mark.parametrize('name', ['partial-9x5', 'full-16x16', 'partial-9x5-aux', 'clamp-alpha-0.999-16x16'])
def test_1_want_abs_equals_an_independent_autograd_statement(name):
    c, r, want, B, A = _built(name)
    if name.startswith('clamp'):
        assert sum(int((tl.al == R.ALPHA_CAP).sum()) for tl in r.blend.tiles) >= 1          # (pixel, entry) pairs at the 0.99 cap
    assert (want > 0).sum() >= 10
    got = _torch_abs(c, r)
    err = np.abs(got - want)
    print(f'{name}: worst |torch - want_abs| / A = {np.where(A > 0, err / np.where(A > 0, A, 1), 0).max():.2e} (bound 1e-10), {int((A > 0).sum())} live elements')
    assert (err <= 1e-10 * A).all()
    assert not got[A == 0].any()


# ---------------------------------------------------------------------------------------------------- 2. properties
@pytest.mark.parametrize('name', ['partial-70x45-deg3', 'aux-all', 'grad-alternate-tiles-zero'])
def test_2_want_abs_lies_between_the_signed_sum_and_the_magnitude(name):
    c, r, want, B, A = _built(name)
    S = r.ref['S'][:, 4:6]
    assert (want >= np.abs(S) - 1e-13 * A).all() and (want <= A * (1 + 1e-13)).all()
    assert not want[A == 0].any() and (want[A > 0] > 0).all()
    assert (A == 0).all(1).sum() > 0                                                         # the case has Gaussians that must get exact zeros
    neg = AR.want_abs(r.blend, *(-a for a in _args(c, r)))
    np.testing.assert_array_equal(neg, want)


def test_2_one_pixel_has_nothing_to_cancel():
    c, r, want, B, A = _built('grad-one-pixel')
    assert (want > 0).sum() > 5
    np.testing.assert_array_equal(want, np.abs(r.ref['S'][:, 4:6]))


# ---------------------------------------------------------------------------------------------------- 3. the test can tell
def test_3_checkerboard_separates_abs_from_signed_by_a_hundred_budgets():
    c, r, want, B, A = _built('partial-70x45-deg3', 'checker')
    assert r.masked == 0
    S = np.abs(r.ref['S'][:, 4:6])
    live = want > 0
    far = (want - S > 100 * B) & live
    print(f'checkerboard: median |S| / abs = {np.median(S[live] / want[live]):.4f}, max B / abs = {(B[live] / want[live]).max():.4f}, '
          f'{int(far.sum())} of {int(live.sum())} live elements further than 100 B from the signed sum')
    assert far.sum() >= 0.5 * live.sum()


# ---------------------------------------------------------------------------------------------------- 4. planted errors
def _planted(c, r):
    """{name: (P, 2)} wrong answers formed from the same addends."""
    P = r.blend.P
    signed, per_block, per_tile, no_wh = (np.zeros((P, 2)) for _ in range(4))
    scale = np.array([0.5 * c.w, 0.5 * c.h])[:, None]
    for tl, i, a, add in AR.addends(r.blend, *_args(c, r)):
        signed[i] += add.sum(1)
        per_tile[i] += np.abs(add.sum(1))
        for b in np.unique(tl.block[a]):
            per_block[i] += np.abs(add[:, a & (tl.block == b)].sum(1))
        no_wh[i] += np.abs(add / scale).sum(1)
    return {'signed sum': np.abs(signed), 'abs after the block sum': per_block, 'abs after the tile sum': per_tile, 'no W/2, H/2': no_wh}


@pytest.mark.parametrize('kind', ['own', 'checker'])
@pytest.mark.parametrize('name', ['partial-70x45-deg3', 'aux-all'])
def test_4_the_judge_rejects_planted_errors(name, kind):
    c, r, want, B, A = _built(name, kind)
    assert AR.judge(want, want, B, A) == (0.0, 0, 0)
    wrong = _planted(c, r)
    wrong['x and y swapped'] = want[:, ::-1].copy()
    np.testing.assert_allclose(wrong['signed sum'], np.abs(r.ref['S'][:, 4:6]), rtol=0, atol=1e-12 * A.max())      # the same addends as BlendRef.sums
    for label, w in wrong.items():
        worst, over, _ = AR.judge(w, want, B, A)
        rows = int((np.abs(w - want) > B).any(1).sum())
        print(f'{name} / {kind} / {label}: {rows} Gaussians over budget, worst err / budget {worst:.3g}')
        assert rows >= 1, label


def test_4_the_judge_counts_a_nonzero_where_zero_is_required():
    c, r, want, B, A = _built('partial-70x45-deg3')
    w = want.copy()
    w[np.flatnonzero((A == 0).all(1))[0], 1] = 1e-30
    assert AR.judge(w, want, B, A)[2] == 1


# ---------------------------------------------------------------------------------------------------- 5. the C ABI
@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, name, **values):
    args = []
    for t, arg in protos[name][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, name)(*args)


def test_5_entry_point_is_declared_and_exported(lib):
    protos = _lib.parse_header()
    name = 'nrc_gs_backward_absgrad_band'
    assert name in protos and hasattr(lib, name)
    assert lib.nrc_abi_version() == _lib.header_abi_version() == 22
    pose = protos['nrc_gs_backward_pose_band'][1]
    mine = protos[name][1]
    assert [a for _, a in mine] == [a for _, a in pose[:-1]] + ['dL_dmean2D_abs', 'stream']
    assert [t.replace(' ', '') for t, _ in mine[-2:]] == ['float*', 'nrc_stream_t']
    assert not any('absgrad' in n and ('rest_step' in n or 'features' in n) for n in protos)


@pytest.mark.parametrize('begin,n', [(-1, 2), (0, 0), (3, 2), (4, 1), (0, 5), (2, -1)])
def test_5_a_bad_band_is_invalid_before_any_device_call(lib, begin, n):
    protos = _lib.parse_header()
    buf = (ctypes.c_float * 16)()
    assert _call(lib, protos, 'nrc_gs_backward_absgrad_band', dL_dmean2D_abs=ctypes.cast(buf, ctypes.c_void_p)) == NRC_ERR_INVALID        # H = 0: no band is valid
    assert _call(lib, protos, 'nrc_gs_backward_absgrad_band', P=0, W=64, H=64, tile_row_begin=begin, n_tile_rows=n,
                 dL_dmean2D_abs=ctypes.cast(buf, ctypes.c_void_p)) == NRC_ERR_INVALID
    assert not any(buf)


def test_5_misaligned_records_are_invalid_before_any_device_call(lib):
    """Host memory stands in for the device buffers: a refused call touches none of them, and no HIP call is made in front of the checks."""
    protos = _lib.parse_header()
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    base += (-base) % 64
    host = (ctypes.c_float * 38)(*([0.0] * 38))
    common = dict(W=64, H=64, tile_row_begin=0, n_tile_rows=4, tan_fovx=0.5, tan_fovy=0.5, camera_dev=ctypes.cast(host, ctypes.c_void_p))
    ptr_args = [a for t, a in protos['nrc_gs_backward_absgrad_band'][1] if '*' in t and a not in ('bg', 'viewmatrix', 'projmatrix', 'campos', 'camera_dev')]
    ptrs = {a: ctypes.c_void_p(base + 64) for a in ptr_args}
    ptrs['pose_partials'] = ptrs['dL_dcamera'] = None
    for off in (4, 16, 32):
        bad = dict(ptrs, grad_records=ctypes.c_void_p(base + 64 + off))
        assert _call(lib, protos, 'nrc_gs_backward_absgrad_band', P=1, **bad, **common) == NRC_ERR_INVALID
    # dL_dcamera without, or with a misaligned, workspace: as in nrc_gs_backward_pose_band
    assert _call(lib, protos, 'nrc_gs_backward_absgrad_band', P=0, dL_dcamera=ctypes.c_void_p(base), dL_dmean2D_abs=ctypes.c_void_p(base + 128), **common) == NRC_ERR_INVALID
    assert _call(lib, protos, 'nrc_gs_backward_absgrad_band', P=0, dL_dcamera=ctypes.c_void_p(base), pose_partials=ctypes.c_void_p(base + 4),
                 dL_dmean2D_abs=ctypes.c_void_p(base + 128), **common) == NRC_ERR_INVALID
    # P == 0: accepted, nothing is launched and nothing is written
    assert _call(lib, protos, 'nrc_gs_backward_absgrad_band', P=0, dL_dmean2D_abs=ctypes.c_void_p(base + 128), **common) == NRC_OK
    assert not any(buf)
