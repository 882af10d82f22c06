"""GPU: the hash-grid TABLE gradient on every backward path (nerficg_amd/csrc/ngp_net.hip: k_grid_bwd, k_grid_bwd_owned, k_grid_bwd_owned_q, k_gb_split +
k_gb_accumulate, k_grid_bwd_general) through the C ABI, every (entry, feature) against the float64 restatement of tests/grid_table_grad_ref.py within its
own budget (derivation there); a value no sample lands on must come back with the bits it went in with.  No entry is excluded and every case checks that
every level has entries with addends.  Each test prints its worst error / budget per path."""
import functools

import numpy as np
import pytest
import torch

from nerficg_amd import _lib
from tests import grid_table_grad_ref as R
from tests import input_grad_ref as I

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
PLS = I.PLS


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a, order='C'))   # (a copy: the cached inputs are read-only)
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _routing(cfg, m, pair_major, workspace):
    """the path every level takes in grid_backward_impl (ngp_net.hip), restated: bucketed with a workspace, slice owners without, atomics below 16 384 rows,
    for sample-major gradients and for the levels the other two leave"""
    _, offsets, _, res = R._layout(cfg)
    L = cfg['n_levels']
    size = np.diff(offsets)
    hashed = [int(res[l]) ** 3 > int(size[l]) for l in range(L)]
    path = ['atomics'] * L
    if not (pair_major and m >= 16384):
        return path
    if workspace:
        first, units = L, 0
        for l in range(L - 1, -1, -1):
            if not hashed[l] or size[l] < 8192 or size[l] % 8192 or res[l] + 1 >= 8192 or units + size[l] // 8192 > 1024:
                break
            units += size[l] // 8192
            first = l
        if first < L:
            return path[:first] + ['bucketed'] * (L - first)
    first, units = L, 0
    for l in range(L - 1, -1, -1):
        c = -(-int(size[l]) // 16384)
        if not hashed[l] or units + c > 256:
            break
        units += c
        first = l
    sparse = all(res[l] + 1 < 16384 and size[l] >= 16384 for l in range(first, L))
    return path[:first] + ['owned_q' if sparse else 'owned'] * (L - first)


def _judge(tag, got, cfg, x, d, path, capacity, old=None, live=None, need_addends=True, ref=None):
    """every entry against the budget of its level's path; returns {path: worst error / budget}"""
    G, A, n = ref if ref is not None else _reference(cfg, x, d, live)
    _, offsets, _, _ = R._layout(cfg)
    assert not need_addends or R.levels_have_addends(n, cfg), tag
    worst = {}
    for l, p in enumerate(path):
        sl = slice(int(offsets[l]), int(offsets[l + 1]))
        o = None if old is None else old[sl]
        if p == 'bucketed':
            budget = R.budget_bucketed(A[sl], n[sl], R.fixed_point_lsb(d, cfg, l, capacity, live), o)
        else:
            budget = R.budget_f32(A[sl], n[sl], o, R.OWN_OLD if p.startswith('owned') else R.ATOMIC_OLD)
        ratio, over, moved = R.judge(got[sl], G[sl], n[sl], budget, o)
        worst[p] = max(worst.get(p, 0.0), ratio)
        assert moved == 0, f'{tag}: level {l} ({p}): {moved} values without an addend changed'
        if over:
            err = np.abs(got[sl].astype(np.float64) - (G[sl] if o is None else G[sl] + o.astype(np.float64)))
            e, f = np.unravel_index(np.argmax(np.where(n[sl] > 0, err / np.maximum(budget, 1e-300), 0.0)), err.shape)
            raise AssertionError(f'{tag}: level {l} ({p}): {over} values over budget, worst {ratio:.3g} x at entry {int(offsets[l]) + e} feature {f}: got '
                                 f'{got[sl][e, f]!r}, want {G[sl][e, f]!r}, n {n[sl][e, f]}, A {A[sl][e, f]!r}')
    print(f'{tag}: worst error / budget ' + ', '.join(f'{p} {r:.3f}' for p, r in worst.items()))
    return worst


_REF: dict = {}


def _reference(cfg, x, d, live):
    """(G, A, n) float64, computed once per input set (keyed by the arrays' identity: the inputs below are cached and read-only)"""
    key = (id(x), id(d), live, tuple(sorted(cfg.items())))
    if key not in _REF:
        out = R.table_grad(x, d, cfg, live)
        for a in out:
            a.setflags(write=False)
        _REF[key] = (out, x, d)   # the arrays are kept alive with their ids
    return _REF[key][0]


@functools.lru_cache(maxsize=None)
def _inputs(n_levels, n_features, log2_t, base, m, seed=0):
    cfg = R.grid_cfg(n_levels, n_features, log2_t, base)
    x = I.positions(m, seed=1000 * log2_t + m + seed)
    d = R.upstream(m, cfg, seed=7 * m + log2_t + base + seed)
    x.setflags(write=False)
    d.setflags(write=False)
    return cfg, x, d


def _device_gradient(cfg, d, pair_major):
    """(M, L F) -> the layout the tuned kernels read: pair-major [L][M][2] or sample-major (M, 2 L)"""
    m = d.shape[0]
    return T(d.reshape(m, cfg['n_levels'], 2).transpose(1, 0, 2)) if pair_major else T(d)


def _old_pattern(cfg):
    """a non-zero table of mixed signs and magnitudes (never -0.0)"""
    rng = np.random.default_rng(5)
    old = (rng.normal(size=(R.n_entries(cfg), cfg['n_features'])) * 10.0 ** rng.uniform(-5, -1, size=(R.n_entries(cfg), 1))).astype(np.float32)
    old[old == 0] = np.float32(1e-3)
    return old


def _run_tuned(cfg, x, d, pair_major, workspace, old=None, live=None, x_dev=None, d_dev=None):
    lib = _lib.load()
    m = x.shape[0] if x_dev is None else x_dev.shape[0]
    args = (cfg['n_levels'], cfg['log2_hashmap_size'], cfg['base_resolution'], cfg['per_level_scale'])
    x_dev = T(x) if x_dev is None else x_dev
    d_dev = _device_gradient(cfg, d, pair_major) if d_dev is None else d_dev
    ws = torch.empty(int(lib.nrc_grid_backward_ws_bytes(m, *args)), dtype=torch.uint8, device=DEV) if workspace else None
    out = torch.zeros(R.n_entries(cfg), 2, device=DEV) if old is None else T(old)
    if live is None:
        _lib.check(lib.nrc_grid_backward(_lib.ptr(x_dev), m, _lib.ptr(d_dev), int(pair_major), *args, _lib.ptr(out), _lib.ptr(ws), _lib.stream_of(out)), 'grid_backward')
    else:
        n_dev = torch.tensor([live, 0], dtype=torch.int32, device=DEV)
        _lib.check(lib.nrc_grid_backward_live(_lib.ptr(x_dev), m, _lib.ptr(d_dev), int(pair_major), *args, _lib.ptr(out), _lib.ptr(ws), _lib.ptr(n_dev),
                                              _lib.stream_of(out)), 'grid_backward_live')
    return out.cpu().numpy()


def _run_general(cfg, x, d, old=None):
    lib = _lib.load()
    m, width = x.shape[0], cfg['n_levels'] * cfg['n_features']
    full = np.full((m, 32), np.nan, np.float32)   # the columns behind the grid's: never read
    full[:, :width] = d
    out = torch.zeros(R.n_entries(cfg), cfg['n_features'], device=DEV) if old is None else T(old)
    x_dev, d_dev = T(x), T(full)
    _lib.check(lib.nrc_grid_backward_general(_lib.ptr(x_dev), m, _lib.ptr(d_dev), cfg['n_levels'], cfg['n_features'], cfg['log2_hashmap_size'],
                                             cfg['base_resolution'], cfg['per_level_scale'], _lib.ptr(out), _lib.stream_of(out)), 'grid_backward_general')
    return out.cpu().numpy()


# ---- A: run-aggregated atomics ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,pair_major', [(m, p) for m in (1, 63, 64, 65, 257, 16383) for p in (True, False)] + [(16384, False)])
def test_atomics_path_every_entry_within_its_budget(m, pair_major):
    cfg, x, d = _inputs(16, 2, 14, 16, m)
    path = _routing(cfg, m, pair_major, True)
    assert set(path) == {'atomics'}
    got = _run_tuned(cfg, x, d, pair_major, workspace=True)
    _judge(f'A M={m} pair-major={pair_major}', got, cfg, x, d, path, m)


# ---- B: slice owners (no workspace) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('log2_t,kernel', [(13, 'owned'), (14, 'owned_q'), (15, 'owned_q')])
def test_ownership_paths_every_entry_within_its_budget(log2_t, kernel):
    """T 2^13: k_grid_bwd_owned with a partial slice (8 192 of 16 384 entries); 2^14: k_grid_bwd_owned_q, one slice per level; 2^15: two"""
    cfg, x, d = _inputs(16, 2, log2_t, 16, 16384)
    path = _routing(cfg, 16384, True, False)
    assert kernel in path and set(path) <= {'atomics', kernel}
    got = _run_tuned(cfg, x, d, True, workspace=False)
    _judge(f'B T=2^{log2_t}', got, cfg, x, d, path, 16384)


# ---- C: bucketed ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('log2_t', [13, 14, 15])            # 1 / 2 / 4 buckets per level
@pytest.mark.parametrize('m', [16384, 16385, 18000])         # 16 385: the last split workgroup holds one sample
def test_bucketed_path_every_entry_within_its_budget(m, log2_t):
    cfg, x, d = _inputs(16, 2, log2_t, 16, m)
    path = _routing(cfg, m, True, True)
    assert 'bucketed' in path and 'atomics' in path
    got = _run_tuned(cfg, x, d, True, workspace=True)
    _judge(f'C M={m} T=2^{log2_t}', got, cfg, x, d, path, m)


# ---- D: sixteen bucketed levels, one split workgroup with 65 536 records and an empty last bucket -----------------------------------------------------------
def _yz_with_all_finest_pairs_in_chunk_0(cfg, seed):
    """(y, z) multiples of 2^-20 whose four (y, z) corner pairs on the finest level all hash into the level's first 8 192-entry slice"""
    _, offsets, scales, _ = R._layout(cfg)
    mask = np.uint32(int(offsets[-1] - offsets[-2]) - 1)
    rng = np.random.default_rng(seed)
    p = (rng.integers(0, 2 ** 20 + 1, size=(4096, 3)).astype(np.float64) / 2.0 ** 20).astype(np.float32)   # columns 1, 2 are y, z
    cell, _ = R._cells(p, scales[-1])
    ty0, tz0 = cell[:, 1] * np.uint32(2654435761), cell[:, 2] * np.uint32(805459861)
    ok = np.ones(4096, bool)
    for a in (ty0, ty0 + np.uint32(2654435761)):
        for b in (tz0, tz0 + np.uint32(805459861)):
            ok &= ((a ^ b) & mask) >> np.uint32(13) == 0
    if ok.any():
        return float(p[ok][0, 1]), float(p[ok][0, 2])
    raise AssertionError('no such (y, z)')


@functools.lru_cache(maxsize=None)
def _inputs_d():
    cfg = R.grid_cfg(16, 2, 14, 32)
    m, block = 16384, 5
    x = I.positions(m, seed=77).copy()
    d = R.upstream(m, cfg, seed=78).copy()
    y, z = _yz_with_all_finest_pairs_in_chunk_0(cfg, seed=79)
    rows = slice(1024 * block, 1024 * (block + 1))
    x[rows, 0] = ((1000 + 1000 * np.arange(1024)) / 2.0 ** 20).astype(np.float32)   # a ray parallel to x
    x[rows, 1], x[rows, 2] = y, z
    d[rows] = R.upstream(1024, cfg, seed=80, zero_rows=0.0)      # live on every level: the workgroup owns 1024 x 4 x 16 records
    assert np.all(d[rows] != 0)
    x.setflags(write=False)
    d.setflags(write=False)
    return cfg, x, d


def test_all_levels_bucketed_with_a_full_split_workgroup():
    """base resolution 32 at T 2^14: every level is hashed and bucketed (two slices each).  Split workgroup 5 is live on all 16 levels with all 1 024
    samples, so its region holds exactly 65 536 records, and none of them falls into the last bucket (the finest level's second slice): that empty
    run starts at record 65 536, one past what the 16-bit start field of the bucket table holds."""
    cfg, x, d = _inputs_d()
    path = _routing(cfg, 16384, True, True)
    assert path == ['bucketed'] * 16
    got = _run_tuned(cfg, x, d, True, workspace=True)
    _judge('D all levels bucketed', got, cfg, x, d, path, 16384)


# ---- E: dynamic range ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs_e():
    cfg = R.grid_cfg(16, 2, 14, 16)
    m = 16384
    x = I.positions(m, seed=91)
    d = R.upstream(m, cfg, seed=92, level_scale=10.0 ** (3.0 - 33.0 * np.arange(16) / 15.0)).copy()   # level maxima ~1e3 (coarsest) ... ~1e-30 (finest)
    small = (d != 0) & (np.abs(d) < np.float32(2.0 ** -120))
    d[small] = np.copysign(np.float32(2.0 ** -120), d[small])    # no denormal INPUTS: what a kernel does with those is not this test's subject
    x.setflags(write=False)
    d.setflags(write=False)
    return cfg, x, d


@pytest.mark.parametrize('pair_major,workspace', [(False, False), (True, False), (True, True)], ids=['atomics', 'owned', 'bucketed'])
def test_level_maxima_from_1e_minus_30_to_1e3_on_every_path(pair_major, workspace):
    """each path against its own budget; on the bucketed levels whose largest gradient lies below 2^-(65 + e_cnt) the fixed-point scale must stay finite"""
    cfg, x, d = _inputs_e()
    path = _routing(cfg, 16384, pair_major, workspace)
    assert (('bucketed' if workspace else 'owned_q') if pair_major else 'atomics') in path
    got = _run_tuned(cfg, x, d, pair_major, workspace)
    assert np.all(np.isfinite(got))
    _judge(f'E pair-major={pair_major} workspace={workspace}', got, cfg, x, d, path, 16384)


# ---- F: positions -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs_f():
    cfg = R.grid_cfg(16, 2, 14, 16)
    rng = np.random.default_rng(17)
    corners = np.stack(np.meshgrid(*[np.array([0.0, 1.0 / 16, 0.5, 15.0 / 16, 1.0])] * 3, indexing='ij'), -1).reshape(-1, 3)    # 125: faces, cell corners
    cluster = (np.array([300000, 700001, 123300]) + rng.integers(0, 400, size=(3000, 3))) / 2.0 ** 20            # inside one finest cell (2^-11 wide)
    rays = []
    while sum(len(r) for r in rays) < 16384:   # short and long rays, ends at every lane position; equal cells in runs on the coarse levels
        o, v = rng.random(3) * 0.3 + 0.1, np.abs(rng.normal(size=3))
        rays.append(o + v / np.linalg.norm(v) * (np.arange(rng.integers(3, 131))[:, None] * (1.7 / 1024)))
    x = R.quantise(np.concatenate([corners, cluster] + rays))
    m = x.shape[0]
    d = R.upstream(m, cfg, seed=18, zero_rows=0.2).copy()        # dead samples inside the runs
    first_ray = 125 + 3000
    d[first_ray + (63 - first_ray) % 64] = 1.0                  # lane 63 of its wave is live, whatever follows it
    x.setflags(write=False)
    d.setflags(write=False)
    return cfg, x, d


@pytest.mark.parametrize('pair_major,workspace', [(False, False), (True, True)], ids=['atomics', 'bucketed'])
def test_faces_corners_one_crowded_cell_and_samples_along_rays(pair_major, workspace):
    cfg, x, d = _inputs_f()
    m = x.shape[0]
    path = _routing(cfg, m, pair_major, workspace)
    assert ('bucketed' in path) == workspace
    _, _, n = _reference(cfg, x, d, None)
    assert n.max() >= 2000    # the crowded cell
    got = _run_tuned(cfg, x, d, pair_major, workspace)
    _judge(f'F M={m} pair-major={pair_major} workspace={workspace}', got, cfg, x, d, path, m)


# ---- G: live count on the bucketed path -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('live', [0, 1, 16383, 16384])
def test_bucketed_path_honours_the_live_count(live):
    cap = 17408
    cfg, x, d = _inputs(16, 2, 14, 16, cap, seed=3)
    xg = x.copy()
    xg[live:] = np.nan
    dg = d.copy()
    dg[live:] = 3e38
    path = _routing(cfg, cap, True, True)
    assert 'bucketed' in path
    got = _run_tuned(cfg, x, d, True, True, live=live, x_dev=T(xg), d_dev=_device_gradient(cfg, dg, True))
    assert np.all(np.isfinite(got))
    _judge(f'G live={live}', got, cfg, x, d, path, cap, live=live, need_addends=live > 0)
    assert live > 0 or not got.any()


# ---- H: general grids -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 257, 5000])
@pytest.mark.parametrize('n_levels,n_features', [(8, 4), (5, 4), (12, 2)])
def test_general_grid_every_entry_within_its_budget(n_levels, n_features, m):
    cfg, x, d = _inputs(n_levels, n_features, 14, 16, m)
    got = _run_general(cfg, x, d)
    _judge(f'H {n_levels}x{n_features} M={m}', got, cfg, x, d, ['general'] * n_levels, m)


# ---- I: the calls ADD to the table they are given --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['atomics', 'owned_q', 'bucketed', 'general'])
def test_gradient_is_added_to_the_callers_values(case):
    if case == 'general':
        cfg, x, d = _inputs(8, 4, 14, 16, 257)
        old = _old_pattern(cfg)
        got, path, m = _run_general(cfg, x, d, old), ['general'] * 8, 257
    else:
        m = 257 if case == 'atomics' else 16384
        cfg, x, d = _inputs(16, 2, 14, 16, m)
        old = _old_pattern(cfg)
        path = _routing(cfg, m, True, case == 'bucketed')
        assert case in path
        got = _run_tuned(cfg, x, d, True, workspace=case == 'bucketed', old=old)
    _judge(f'I {case}', got, cfg, x, d, path, m, old=old)


# ---- the module: tinycudann.NetworkWithInputEncoding's routing (tuned or general kernel, layout, workspace) -------------------------------------------------
NET_D = {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': 'None', 'n_neurons': 64, 'n_hidden_layers': 1}


@pytest.mark.parametrize('n_levels,n_features,log2_t,m', [(16, 2, 19, 5000), (16, 2, 19, 20011), (8, 4, 19, 5000), (5, 4, 14, 5000)])
def test_module_table_gradient_under_the_identity_probe(n_levels, n_features, log2_t, m):
    """The identity-probe weights of test_grid_encoding_alone_bit_level: W0 = [I ; 0], output column l reads hidden neuron l F (feature 0 of level l), a
    positive table keeps every ReLU open.  The upstream gradients are fp16 values in [2^-13, 2) whose product with the internal loss scale 128 is exact in
    fp16, every sum of the MLP backward has ONE non-zero term, and the unscaling is a power of two: d_in[:, l F] is the upstream column l exactly and every
    other column is 0, so params.grad behind the MLP part is held to the same budgets as the C ABI calls -- and the features nothing flows to stay 0."""
    import nerficg_amd.tinycudann as tcnn
    cfg = R.grid_cfg(n_levels, n_features, log2_t)
    enc = {'otype': 'Grid', 'type': 'Hash', 'n_levels': n_levels, 'n_features_per_level': n_features, 'log2_hashmap_size': log2_t, 'base_resolution': 16,
           'per_level_scale': PLS, 'interpolation': 'Linear'}
    net = tcnn.NetworkWithInputEncoding(3, 16, enc, NET_D, seed=5).to(DEV)
    n_in = net.n_in_padded
    assert net.n_mlp_params == 64 * n_in + 16 * 64 and net.params.numel() == net.n_mlp_params + R.n_entries(cfg) * n_features
    with torch.no_grad():
        w0 = torch.zeros(64, n_in)
        w0[:n_in] = torch.eye(n_in)
        wo = torch.zeros(16, 64)
        wo[torch.arange(n_levels), torch.arange(n_levels) * n_features] = 1.0
        net.params[:net.n_mlp_params] = torch.cat([w0.reshape(-1), wo.reshape(-1)]).to(DEV)
        gen = torch.Generator().manual_seed(3)
        net.params[net.n_mlp_params:] = (0.25 + 0.5 * torch.rand(net.params.numel() - net.n_mlp_params, generator=gen)).to(DEV)
    rng = np.random.default_rng(m + n_levels)
    x = I.positions(m, seed=m + log2_t)
    g = ((1.0 + rng.integers(0, 1024, size=(m, 16)) / 1024.0) * 2.0 ** rng.integers(-13, 1, size=(m, 16)) * rng.choice([-1.0, 1.0], size=(m, 16))).astype(np.float16)
    dead = rng.random(m) < 0.25
    dead[0] = False
    g[dead] = 0
    g[:, n_levels:] = 0
    assert np.all((g.astype(np.float32) * 128).astype(np.float16).astype(np.float32) == g.astype(np.float32) * 128)
    d = np.zeros((m, n_levels * n_features), np.float32)
    d[:, ::n_features] = g[:, :n_levels].astype(np.float32)
    out = net(T(x))
    out.backward(T(g))
    got = net.params.grad[net.n_mlp_params:].reshape(-1, n_features).cpu().numpy()
    path = _routing(cfg, m, True, True) if (n_levels, n_features) == (16, 2) else ['general'] * n_levels
    assert (m < 16384) == ('bucketed' not in path)
    _judge(f'module {n_levels}x{n_features} T=2^{log2_t} M={m}', got, cfg, x, d, path, m, ref=R.table_grad(x, d, cfg))   # (not kept: 300 MB at T = 2^19)
    assert n_features == 1 or not got[:, 1:].any()
