"""CPU: the per-Gaussian contribution statistics of the 3DGS rasterizer -- the reference the GPU tests rely on (tests/gs_contrib_ref.py) against an independent
per-pixel loop and two identities, the C ABI of the entry point (exported, declared, every refused call refused before any HIP call), and the host logic of
Gaussians.prune_by_contribution with a stub in place of prune_points."""
import functools

import numpy as np
import pytest
import torch

import oracle
from nerficg_amd import _lib
from tests import gs_contrib_ref as CR
from tests import gs_features_ref as F
from tests import gs_grad_cases as GC
from tests import gs_grad_ref as R

SYMBOL = 'nrc_gs_contributions_band'
NRC_OK, NRC_ERR_INVALID = 0, -1
f64 = np.float64


# ---------------------------------------------------------------------------------------------------- the reference, on the oracle alone
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(case, float64 oracle state, BlendRef).  'partial-9x5': 300 Gaussians on 45 pixels, most of them listed and far below 1/255;
    'opaque-20x18': every third Gaussian at opacity 0.999 (alpha clamps at 0.99) on 2 x 2 partial tiles -- pixels saturate and stop early."""
    c = GC.get('partial-9x5') if name == 'partial-9x5' else GC._case(name, GC._opaque_third(), w=20, h=18)
    sc, cam = c.sc, c.cam
    cast = lambda a: np.asarray(a, f64)
    _, _, st = oracle.gs_forward(cast(sc['means3D']), cast(sc['opacities']), cast(cam['viewmatrix']), cast(cam['projmatrix']), cast(cam['campos']), cam['tanfovx'],
                                 cam['tanfovy'], c.w, c.h, np.zeros(3, f64), sh_degree=sc['sh_degree'], shs=cast(sc['shs']), scales=cast(sc['scales']),
                                 rotations=cast(sc['rotations']), dtype=f64)
    return c, st, R.BlendRef(st, np.zeros(3))


@pytest.mark.parametrize('name', ['partial-9x5', 'opaque-20x18'])
@pytest.mark.parametrize('mapped', [False, True])
def test_reference_equals_a_brute_force_pixel_loop(name, mapped):
    c, st, blend = _scene(name)
    m = CR.random_map(blend, seed=1) if mapped else np.ones((c.h, c.w), np.float32)     # ambiguous pixels stay in: both sides are float64 on the same decisions
    ref = CR.ContribRef(blend, m)
    ws, wm, hits, Tf = CR.brute_force(st, m)
    assert hits.sum() > 0 and np.array_equal(ref.hits, hits)
    assert (np.abs(ref.weight_sum - ws) <= 1e-12 * ref.A).all() and (np.abs(ref.weight_max - wm) <= 1e-14).all()
    assert (np.abs(blend.T_final - Tf) <= 1e-14).all()
    assert ((ref.A > 0) == (hits > 0)).all() and ((ref.weight_max > 0) == (hits > 0)).all()
    assert (ref.B[hits > 0] > 0).all() and (ref.B_max[hits > 0] > 0).all() and not ref.B[hits == 0].any()
    # what the scenes are for
    ranges, ncon = np.asarray(st.ranges).astype(np.int64), np.asarray(st.n_contrib).reshape(c.h, c.w)
    listed = np.unique(np.concatenate([np.asarray(st.point_list)[a:b] for a, b in ranges]))
    if not mapped:
        assert (hits[listed] == 0).any(), 'no Gaussian is listed but never blended'
    if name == 'opaque-20x18':
        gx = (c.w + 15) // 16
        length = np.array([[ranges[(y // 16) * gx + x // 16][1] - ranges[(y // 16) * gx + x // 16][0] for x in range(c.w)] for y in range(c.h)])
        assert ((ncon < length) & (Tf < 1e-4 / 0.01)).any(), 'no pixel terminates early'
    if mapped:
        assert (m == 0).any() and (hits < CR.brute_force(st, np.ones_like(m))[2]).any()


@pytest.mark.parametrize('name', ['partial-9x5', 'opaque-20x18'])
def test_identities(name):
    c, st, blend = _scene(name)
    ones = np.ones((c.h, c.w), np.float32)
    ref = CR.ContribRef(blend, ones)
    total, want = ref.weight_sum.sum(), (1.0 - blend.T_final).sum()
    print(f'{name}: sum_i weight_sum = {total!r}, sum_p (1 - T_final) = {want!r}')
    assert abs(total - want) <= 1e-12 * want                           # every pixel's weights telescope to 1 - T_final
    m = CR.participation(blend, CR.random_map(blend, seed=2))
    ref = CR.ContribRef(blend, m)
    SF = F.FeatureRef(blend, np.ones((c.n, 1), np.float32)).sums(m[None])['SF'][:, 0]
    assert (np.abs(ref.weight_sum - SF) <= 1e-12 * ref.A).all() and ref.A.sum() > 0


# ---------------------------------------------------------------------------------------------------- the C ABI, without a GPU
@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, **values):
    """The entry point with null pointers and zeros everywhere except the named arguments (tests/test_gs_features_ref_cpu.py)."""
    args = []
    for t, arg in protos[SYMBOL][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, SYMBOL)(*args)


ADDR = 0x10000   # a fake non-null address, 64-byte aligned: a refused call must not touch it


def _valid(**change):
    v = dict(P=10, W=64, H=64, tile_row_begin=0, n_tile_rows=4, point_list=ADDR, ranges=ADDR, splat_records=ADDR, tile_order=ADDR, n_contrib=ADDR,
             weight_sum=ADDR, weight_max=ADDR, hits=ADDR)
    v.update(change)
    return v


def test_entry_point_is_exported_and_declared(lib):
    protos = _lib.parse_header()
    assert SYMBOL in protos and hasattr(lib, SYMBOL)
    names = [a for _, a in protos[SYMBOL][1]]
    assert names == ['P', 'W', 'H', 'point_list', 'ranges', 'splat_records', 'tile_order', 'n_contrib', 'pixel_weights', 'weight_sum', 'weight_max', 'hits', 'clear',
                     'tile_row_begin', 'n_tile_rows', 'stream']
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 21


@pytest.mark.parametrize('begin,n', [(-1, 2), (0, 0), (3, 2), (4, 1), (0, 5), (2, -1)])
def test_a_bad_band_is_invalid_before_any_device_call(lib, begin, n):
    """H = 64: four tile rows.  Everything else about the call is valid, and no GPU is needed for the answer."""
    protos = _lib.parse_header()
    assert _call(lib, protos) == NRC_ERR_INVALID                                          # H = 0: no band is valid
    assert _call(lib, protos, **_valid(tile_row_begin=begin, n_tile_rows=n)) == NRC_ERR_INVALID


@pytest.mark.parametrize('change', [dict(point_list=None), dict(splat_records=None), dict(ranges=None), dict(tile_order=None), dict(n_contrib=None), dict(P=-1), dict(W=0),
                                    dict(weight_sum=None, weight_max=None, hits=None), dict(splat_records=ADDR + 4), dict(splat_records=ADDR + 8),
                                    dict(weight_sum=ADDR + 2), dict(hits=ADDR + 1), dict(pixel_weights=ADDR + 3)])
def test_null_lists_misaligned_records_and_no_output_are_invalid(lib, change):
    protos = _lib.parse_header()
    assert _call(lib, protos, **_valid(**change)) == NRC_ERR_INVALID


def test_no_gaussians_is_ok_without_a_launch(lib):
    """P == 0 returns before any HIP call, so it answers on a machine without a GPU as well; the lists may then be null."""
    protos = _lib.parse_header()
    assert _call(lib, protos, **_valid(P=0, point_list=None, splat_records=None, weight_max=None)) == NRC_OK


# ---------------------------------------------------------------------------------------------------- prune_by_contribution, host logic
def _model(P=8):
    from nerficg_amd.gaussian_splatting import Gaussians
    g = Gaussians(torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 4), torch.zeros(P, 1), torch.zeros(P, 1, 3), torch.zeros(P, 15, 3))
    calls = []
    g.prune_points = lambda mask: calls.append(mask.clone())            # the stub: records the mask
    return g, calls


STATS = dict(weight_sum=torch.tensor([5.0, 1.0, 3.0, 3.0, 0.0, 9.0, 3.0, 0.5]), weight_max=torch.tensor([0.9, 0.02, 0.3, 0.005, 0.0, 0.99, 0.3, 0.2]),
             hits=torch.tensor([40, 3, 12, 1, 0, 77, 9, 2], dtype=torch.int32))


@pytest.mark.parametrize('kw,pruned', [
    (dict(min_weight_max=0.01), [3, 4]),
    (dict(min_hits=1), [4]),
    (dict(min_hits=3), [3, 4, 7]),
    (dict(keep_fraction=0.5), [1, 4, 7]),                # k = 4: the 4th largest weight_sum is 3.0 and all three 3.0 rows stay (ties kept): five are kept
    (dict(keep_fraction=0.25), [1, 2, 3, 4, 6, 7]),
    (dict(keep_fraction=1.0), []),
    (dict(keep_fraction=0.0), [0, 1, 2, 3, 4, 5, 6, 7]),
    (dict(min_weight_max=0.25, min_hits=10), [1, 3, 4, 6, 7]),
    (dict(min_hits=2, keep_fraction=0.75), [3, 4, 7]),   # k = 6: the 6th largest is 1.0 -> rows 4 and 7 by the score, 3 and 4 by the hits
])
def test_prune_by_contribution_masks(kw, pruned):
    g, calls = _model()
    out = g.prune_by_contribution(STATS, **kw)
    assert out == {'pruned': len(pruned), 'kept': 8 - len(pruned)}
    if pruned:
        assert len(calls) == 1 and calls[0].dtype == torch.bool and calls[0].nonzero().flatten().tolist() == pruned
    else:
        assert not calls


def test_prune_by_contribution_refuses_no_criterion_and_foreign_statistics():
    g, calls = _model()
    with pytest.raises(ValueError, match='at least one'):
        g.prune_by_contribution(STATS)
    other = {k: v[:-1] for k, v in STATS.items()}
    for kw in (dict(min_hits=1), dict(min_weight_max=0.1), dict(keep_fraction=0.5)):
        with pytest.raises(ValueError, match='8 Gaussians'):
            g.prune_by_contribution(other, **kw)
    with pytest.raises(ValueError, match='keep_fraction'):
        g.prune_by_contribution(STATS, keep_fraction=1.5)
    with pytest.raises(ValueError, match='hits'):
        g.prune_by_contribution(dict(weight_sum=STATS['weight_sum']), min_hits=1)
    assert not calls
