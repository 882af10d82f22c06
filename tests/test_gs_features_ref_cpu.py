"""CPU: the feature pass of the 3DGS rasterizer -- the C ABI of its two entry points (exported, declared, every refused call refused before any HIP call),
and the reference the GPU tests rely on (tests/gs_features_ref.py), checked on the oracle alone:

  * the reference module equals ceil(C / 3) independent runs of the float64 oracle with colors_precomp triples and background 0, map and gradients;
  * the assembled gradient of <g, feature_map> equals a float64 central difference for mean3D, opacity and feature entries;
  * the float32 oracle's serial sums lie inside the order='serial' form of the budget (the budget is not too tight)."""
import functools

import numpy as np
import pytest

import oracle
from nerficg_amd import _lib
from tests import gs_features_ref as F
from tests import gs_grad_cases as GC
from tests import gs_grad_ref as R

SYMBOLS = ('nrc_gs_render_features_band', 'nrc_gs_backward_features_band')
NRC_ERR_INVALID = -1
f64 = np.float64


@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, name, **values):
    """The entry point with null pointers and zeros everywhere except the named arguments (tests/test_gs_bands_cpu.py)."""
    args = []
    for t, arg in protos[name][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, name)(*args)


def test_feature_entry_points_are_exported_and_declared(lib):
    protos = _lib.parse_header()
    for name in SYMBOLS:
        assert name in protos and hasattr(lib, name), name
        names = [a for _, a in protos[name][1]]
        assert names[:5] == ['P', 'C', 'W', 'H', 'features'] and names[-1] == 'stream' and 'tile_row_begin' in names and 'n_tile_rows' in names
    assert 'records_clear' in [a for _, a in protos[SYMBOLS[1]][1]]
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 20
    assert not any('rest_step' in n and 'features' in n for n in protos)                  # no feature form of the in-backward Adam step


# fake non-null addresses: a refused call must not touch them (64-byte aligned unless a case says otherwise)
ADDR = 0x10000


def _valid(name):
    v = dict(P=10, C=5, W=64, H=64, tile_row_begin=0, n_tile_rows=4, features=ADDR, point_list=ADDR, ranges=ADDR, splat_records=ADDR, tile_order=ADDR, n_contrib=ADDR)
    if name == SYMBOLS[0]:
        v.update(out_features=ADDR)
    else:
        v.update(final_T=ADDR, dL_dfeature_map=ADDR, dL_dfeatures=ADDR, grad_records=ADDR)
    return v


@pytest.mark.parametrize('name', SYMBOLS)
@pytest.mark.parametrize('begin,n', [(-1, 2), (0, 0), (3, 2), (4, 1), (0, 5), (2, -1)])
def test_a_bad_band_is_invalid_before_any_device_call(lib, name, begin, n):
    """H = 64: four tile rows.  Everything else about the call is valid, and no GPU is needed for the answer."""
    protos = _lib.parse_header()
    assert _call(lib, protos, name) == NRC_ERR_INVALID                                   # H = 0: no band is valid
    v = _valid(name)
    v.update(tile_row_begin=begin, n_tile_rows=n)
    assert _call(lib, protos, name, **v) == NRC_ERR_INVALID


@pytest.mark.parametrize('name', SYMBOLS)
@pytest.mark.parametrize('change', [dict(C=0), dict(C=-3), dict(C=257), dict(features=None), dict(P=-1)])
def test_a_bad_channel_count_or_null_features_is_invalid(lib, name, change):
    protos = _lib.parse_header()
    v = _valid(name)
    v.update(change)
    assert _call(lib, protos, name, **v) == NRC_ERR_INVALID


def test_misaligned_records_are_invalid(lib):
    protos = _lib.parse_header()
    for off in (4, 16, 32):
        v = _valid(SYMBOLS[1])
        v.update(grad_records=ADDR + off)
        assert _call(lib, protos, SYMBOLS[1], **v) == NRC_ERR_INVALID
    for name in SYMBOLS:
        v = _valid(name)
        v.update(splat_records=ADDR + 4)
        assert _call(lib, protos, name, **v) == NRC_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- the reference, on the oracle alone
def _case(name):
    return GC._case('ref-64x48', w=64, h=48) if name == 'ref-64x48' else GC.get(name)


def _oracle_args(c, dtype):
    sc, cam = c.sc, c.cam
    cast = lambda a: np.asarray(a, dtype)
    args = (cast(sc['means3D']), cast(sc['opacities']), cast(cam['viewmatrix']), cast(cam['projmatrix']), cast(cam['campos']), cam['tanfovx'], cam['tanfovy'], c.w, c.h)
    return args, dict(scales=cast(sc['scales']), rotations=cast(sc['rotations']))


def _triple(a, t):
    """Columns 3 t .. 3 t + 2 of a (n, C) array (or planes of a (C, H, W) array), zero-padded."""
    out = np.zeros((3,) + a.shape[1:], a.dtype) if a.ndim == 3 else np.zeros((a.shape[0], 3), a.dtype)
    if a.ndim == 3:
        n = min(3, a.shape[0] - 3 * t)
        out[:n] = a[3 * t:3 * t + n]
    else:
        n = min(3, a.shape[1] - 3 * t)
        out[:, :n] = a[:, 3 * t:3 * t + n]
    return out


def _oracle_runs(c, feats, dtype, overrides=None):
    """ceil(C / 3) independent oracle runs with colors_precomp triples and background 0: [(image (3, H, W), state)]."""
    args, geo = _oracle_args(c, dtype)
    if overrides:
        args = list(args)
        for k, v in overrides.items():
            args[k] = v
    runs = []
    for t in range((feats.shape[1] + 2) // 3):
        img, _, st = oracle.gs_forward(*args, np.zeros(3, dtype), sh_degree=c.sc['sh_degree'], colors_precomp=_triple(np.asarray(feats, dtype), t), dtype=dtype, **geo)
        runs.append((img, st))
    return runs


@pytest.mark.parametrize('name', ['partial-9x5', 'ref-64x48'])
@pytest.mark.parametrize('C', [1, 3, 5, 7])
def test_reference_equals_independent_float64_oracle_runs(name, C):
    c = _case(name)
    feats = F.random_features(c.n, C, seed=C)
    runs = _oracle_runs(c, feats, f64)
    st = runs[0][1]
    blend = R.BlendRef(st, np.zeros(3))
    assert blend.ambiguous.sum() <= 0.005 * c.w * c.h
    fr = F.FeatureRef(blend, feats)
    want, bud, mag = fr.feature_map()
    got = np.concatenate([img for img, _ in runs])[:C]
    print(f'{name} C={C}: map, worst |diff| / A {np.max(np.abs(got - want)[mag > 0] / mag[mag > 0]):.2e}')
    assert (np.abs(got - want) <= 1e-12 * mag).all()
    g = fr.mask_ambiguous(F.random_map_gradients(c, C, seed=C))
    ref = fr.sums(g)
    B, BF = F.budget(ref)
    total = None
    SF = np.zeros((c.n, 3 * len(runs)))
    for t, (_, st_t) in enumerate(runs):
        grads = oracle.gs_backward(st_t, _triple(g, t).astype(f64))
        SF[:, 3 * t:3 * t + 3] = grads['color']
        total = {k: grads[k] if total is None else total[k] + grads[k] for k in ('mean3D', 'mean2D', 'opacity', 'scale', 'rot', 'conic')}
    SF = SF[:, :C]
    assert (np.abs(SF - ref['SF']) <= 1e-9 * ref['AF']).all()
    leaf = F.leaves(c, st, ref, B)
    for k in ('mean3D', 'mean2D', 'opacity', 'scale', 'rot'):
        err = np.abs(total[k].reshape(leaf.want[k].shape) - leaf.want[k])
        live = leaf.A[k] > 0
        print(f'{name} C={C}: {k}, worst err / A {np.max(err[live] / leaf.A[k][live], initial=0.0):.2e}')
        assert (err <= 1e-9 * leaf.A[k]).all(), k
        assert (leaf.budget[k][live] > 0).all()


def test_assembled_gradient_against_a_float64_central_difference():
    """d/dtheta of <g, feature_map> at C = 5 on the 64 x 48 scene, oracle in float64, for three mean3D components, three opacities and three feature entries.
    Observed step error on this scene at h = 1e-6, relative to the largest picked gradient (334.8, a mean3D entry): at most 1.3e-10 for the three mean3D
    entries, 2.0e-11 for the opacities, 1.6e-11 for the feature entries (those are linear in the step: what is left is the float64 rounding part
    eps |f| / h).  The bound is ten times the largest observation: 1.3e-9 relative (OBSERVED_H6 below)."""
    c = _case('ref-64x48')
    C = 5
    feats = F.random_features(c.n, C, seed=1).astype(f64)
    g = F.random_map_gradients(c, C, seed=1)
    runs = _oracle_runs(c, feats, f64)
    blend = R.BlendRef(runs[0][1], np.zeros(3))
    fr = F.FeatureRef(blend, feats.astype(np.float32))
    g = fr.mask_ambiguous(g)
    ref = fr.sums(g)
    leaf = F.leaves(c, runs[0][1], ref, F.budget(ref)[0])
    args, _ = _oracle_args(c, f64)

    def value(means=None, opac=None, f=None):
        over = {}
        if means is not None:
            over[0] = means
        if opac is not None:
            over[1] = opac
        rs = _oracle_runs(c, feats if f is None else f, f64, over)
        return float(sum((img * _triple(g, t)).sum() for t, (img, _) in enumerate(rs)))

    wm, wo, wf = leaf.want['mean3D'], leaf.want['opacity'], ref['SF']
    picks = [('means', (int(i), int(np.argmax(np.abs(wm[i])))), wm) for i in np.argsort(-np.abs(wm).max(1))[:3]]
    picks += [('opac', (int(i),), wo) for i in np.argsort(-np.abs(wo))[:3]]
    picks += [('f', (int(i), int(np.argmax(np.abs(wf[i])))), wf) for i in np.argsort(-np.abs(wf).max(1))[:3]]
    base = dict(means=args[0], opac=args[1], f=feats)
    scale = max(abs(float(w[idx])) for _, idx, w in picks)
    assert scale > 0
    h = 1e-6
    for key, idx, w in picks:
        vals = []
        for sign in (+1.0, -1.0):
            pert = base[key].copy()
            pert[idx] += sign * h
            vals.append(value(**{key: pert}))
        fd = (vals[0] - vals[1]) / (2 * h)
        print(key, idx, 'assembled', float(w[idx]), 'central difference', fd, 'relative', abs(fd - float(w[idx])) / scale)
        assert abs(fd - float(w[idx])) <= 10 * OBSERVED_H6 * scale, (key, idx, fd, float(w[idx]))


OBSERVED_H6 = 1.3e-10   # the run recorded in the docstring above


@functools.lru_cache(maxsize=None)
def _serial(name, C):
    c = _case(name)
    st, _ = GC.forward(c)
    feats = F.random_features(c.n, C, seed=C)
    blend = R.BlendRef(R.promote(st), np.zeros(3))
    fr = F.FeatureRef(blend, feats)
    g = fr.mask_ambiguous(F.random_map_gradients(c, C, seed=C))
    ref = fr.sums(g)
    return c, st, feats, g, fr, ref


@pytest.mark.parametrize('name', ['partial-9x5', 'ref-64x48'])
@pytest.mark.parametrize('C', [1, 3, 5, 7])
def test_float32_oracle_within_the_serial_budget(name, C):
    c, st, feats, g, fr, ref = _serial(name, C)
    B, BF = F.budget(ref, order='serial')
    runs = _oracle_runs(c, feats, np.float32)
    S = np.zeros((c.n, 9))
    SF = np.zeros((c.n, 3 * len(runs)))
    maps = []
    for t, (img, st_t) in enumerate(runs):
        np.testing.assert_array_equal(st_t.n_contrib, st.n_contrib)                     # the blended set does not depend on what is blended
        cols = GC.sums_of(oracle.gs_backward(st_t, _triple(g, t))).astype(f64)
        S[:, 3:] += cols[:, 3:9]
        SF[:, 3 * t:3 * t + 3] = cols[:, :3]
        maps.append(img)
    worst, over, nonzero = R.judge(S, ref['S'], B, ref['A'])
    print(f'{name} C={C}: geometry sums, worst err / budget {worst:.3f}')
    assert over == 0 and nonzero == 0
    worst, over, nonzero = R.judge(SF[:, :C], ref['SF'], BF, ref['AF'])
    print(f'{name} C={C}: feature gradient, worst err / budget {worst:.3f}')
    assert over == 0 and nonzero == 0
    want, bud, mag = fr.feature_map()
    worst, over, nonzero = R.judge(np.concatenate(maps)[:C], want, bud, mag)
    print(f'{name} C={C}: map, worst err / budget {worst:.3f}')
    assert over == 0 and nonzero == 0
