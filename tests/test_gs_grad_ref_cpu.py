"""CPU: the float64 reference and the per-element budgets of the 3DGS backward (tests/gs_grad_ref.py, cases in tests/gs_grad_cases.py) before they judge a kernel.

  * the numpy restatement of the blend backward equals oracle.gs_backward in its double instantiation on the promoted state within 1e-5 A per element
    (measured <= 1.3e-6 A: what is left is the float32 final_T the oracle is handed, the restatement forms its own);
  * the budgets are not too tight: the serial f32 oracle passes `judge` on every case (it uses at most 0.14 of any element's budget);
  * the budgets are not too loose: eight planted errors, applied to the f32 oracle's result, fail `judge` under BOTH budgets (the kernel's order of
    summation and the serial one; the looser of the two per element is used);
  * at most 0.5 % of a case's pixels are ambiguous, and each case contains what it is named for."""
import functools

import numpy as np
import pytest

import oracle
from tests import gs_grad_cases as C
from tests import gs_grad_ref as R
from tests.gs_pose_grad_ref import fov_clamped


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, st, st2, reference with the serial budget, reference budget in the kernel's order): computed once per case, never modified."""
    c = C.get(name)
    st, st2 = C.forward(c)
    r = C.reference(c, st, order='serial')
    return c, st, st2, r, R.blend_budget(r.ref, c.w, c.h, 'kernel')


def _contents(name, c, st, r):
    """Each case contains what it is named for."""
    ref, blend = r.ref, r.blend
    lists = st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0]
    live = ref['gexp'] >= R.BW_E_MIN
    vis = st.radii > 0
    assert (ref['A'][:, 3] > 0).sum() >= 1
    if name.startswith('partial'):
        assert c.w % 16 and c.h % 16
    if name == 'partial-70x45-deg3':
        assert (c.w % 16, c.h % 16) == (6, 13) and ref['tiles'].max() > 1
    if name == 'partial-9x5':
        assert len(blend.tiles) == 1
    if name == 'partial-113x71-2000-deg2':
        assert len(blend.tiles) == 8 * 5 and ref['blocks'].max() > 64
    if name == 'single-wide':
        assert vis.sum() == 1 and ref['tiles'][0] == 4
    if name.startswith('dense'):
        assert lists.max() > 512 and st.n_contrib.max() > 256 and ref['k'].max() > 256           # more than two batches; a chain past a batch
    if name == 'grad-one-pixel':
        assert live.sum() == 1 and (np.abs(r.g).max(0) > 0).sum() == 1 and (ref['A'][:, 3] > 0).sum() > 5
    if name == 'grad-tile-exponents':
        assert np.unique(ref['gexp'][live]).size >= 8 and np.ptp(ref['gexp'][live]) > 30
    if name == 'grad-hot-pixel':
        assert ref['gexp'].max() >= 12 and np.sort(ref['gexp'])[-2] <= 3
    if name == 'grad-2^-70':
        assert live.all() and (ref['gexp'] == R.BW_E_MIN).all() and np.abs(r.g).max() < 2.0 ** -66       # the floor, not the gradients' own exponent
    if name == 'grad-alternate-tiles-zero':
        assert (live == (np.arange(live.size) % 2 == 0)).all()
    if name == 'clamp-sh-dc-x3':
        cl = st.clamped[vis].astype(bool)
        assert cl.sum() > 50 and st.rgb[vis][~cl].min() > 1e-5, (cl.sum(), st.rgb[vis][~cl].min())     # clamp decisions no rounding can move
        assert (r.leaf.A['sh'][vis][:, 0][cl] == 0).all()
    if name == 'clamp-alpha-0.999':
        capped = sum(int((tl.al == R.ALPHA_CAP).sum()) for tl in blend.tiles)
        ncon = st.n_contrib.reshape(c.h, c.w)
        ty, tx = np.meshgrid(np.arange(c.h) // 16, np.arange(c.w) // 16, indexing='ij')
        stopped = int(((ncon < lists[ty * ((c.w + 15) // 16) + tx]) & (blend.T_final < 1e-3)).sum())
        assert capped >= 10 and stopped >= 50, (capped, stopped)            # (pixel, entry) pairs at the 0.99 cap; pixels that stop before their list ends
    if name == 'clamp-fov-radius-1.6':
        fc = fov_clamped(c.sc, c.cam, st)
        assert fc.sum() > 20 and (fc & (ref['A'][:, 3] > 0)).sum() > 5, (fc.sum(), (fc & (ref['A'][:, 3] > 0)).sum())
    if c.aux:
        assert ref['S'].shape[1] == 10 and (np.abs(ref['S'][:, 9]).max() > 0) == (c.aux != 'alpha_only')


@pytest.mark.parametrize('name', list(C.CASES))
def test_restatement_budget_and_contents_of_every_case(name):
    c, st, st2, r, B_kernel = _built(name)
    _contents(name, c, st, r)
    ref = r.ref
    A = ref['A']
    live = A > 0
    # the restatement against the double oracle on the promoted state
    st64 = R.promote(st)
    S64 = C.oracle_sums(c, st64, None if st2 is None else R.promote(st2), r.g, r.g_d, r.g_a)
    err = np.abs(ref['S'] - S64)
    print(f'{name}: restatement vs double oracle, worst err / A {np.max(err[live] / A[live]):.2e}; {r.masked} of {c.w * c.h} pixels masked; '
          f'budget / A median {np.median(r.B[live] / A[live]):.2e} (serial), {np.median(B_kernel[live] / A[live]):.2e} (kernel order)')
    assert (err <= 1e-5 * A).all()
    # the serial f32 oracle within the budgets
    S32 = C.oracle_sums(c, st, st2, r.g, r.g_d, r.g_a)
    worst, over, nonzero = R.judge(S32, ref['S'], r.B, A)
    print(f'{name} blend sums: worst err / budget {worst:.3f}')
    assert over == 0 and nonzero == 0
    for leaf, (worst, over, nonzero) in C.judge_all(c, C.oracle_leaves(c, st, st2, S32), r.leaf).items():
        assert over == 0 and nonzero == 0, (name, leaf, worst, over, nonzero)


# ------------------------------------------------------------------------------------------------------------------------ planted errors
def _loose(name):
    """The case with the LOOSER of the two budgets per element: a planted error that fails here fails under either."""
    c, st, st2, r, B_kernel = _built(name)
    B = np.maximum(r.B, B_kernel)
    leaf = R.LeafRef(r.st64, r.ref, B, view_z=np.asarray(c.cam['viewmatrix'])[:3, 2])
    S32 = C.oracle_sums(c, st, st2, r.g, r.g_d, r.g_a)
    assert R.judge(S32, r.ref['S'], B, r.ref['A'])[1:] == (0, 0)
    return c, st, st2, r, B, leaf, S32.astype(np.float64)


def _rejected(c, st, st2, leaf, S_planted, leaves=None, flags=None):
    """Number of elements `judge` rejects when the f32 oracle's stage 2 runs on the planted sums."""
    st_used = st
    if flags is not None:                                            # a state with other clamp flags, for the oracle's stage 2 only
        st_used = oracle.GSState()
        st_used.__dict__.update(st.__dict__)
        st_used.clamped = flags
    got = C.oracle_leaves(c, st_used, st2, S_planted)
    bad = 0
    for name in (leaves or C.leaf_names(c)):
        worst, over, nonzero = R.judge(got[name], leaf.want[name], leaf.budget[name], leaf.A[name])
        bad += over + nonzero
    return bad


def _typical(S, A, q):
    """A Gaussian whose sum q is not a deep cancellation: the median |S| among those with |S| >= A / 50 (1 % of that is 2e-4 A; mean2D sums of random
    pixel gradients rarely keep more)."""
    ok = np.flatnonzero((A[:, q] > 0) & (np.abs(S[:, q]) >= 0.02 * A[:, q]))
    assert ok.size >= 5
    return ok[np.argsort(np.abs(S[ok, q]))[ok.size // 2]]


def test_planted_one_tile_of_a_gaussian_missing():
    c, st, st2, r, B, leaf, S32 = _loose('partial-70x45-deg3')
    i = int(np.argmax(r.ref['tiles']))
    assert r.ref['tiles'][i] >= 4
    # the tile that gives this Gaussian the LEAST: its share is the difference of the reference with that tile's gradients zeroed
    shares = []
    for tl in r.blend.tiles:
        if i in tl.ids:
            g = r.g.copy()
            g[:, tl.py, tl.px] = 0
            shares.append(r.ref['S'][i] - r.blend.sums(g)['S'][i])
    shares = [s for s in shares if np.abs(s).max() > 0]
    assert len(shares) >= 4
    share = min(shares, key=lambda s: np.abs(s).max())
    S = S32.copy()
    S[i] -= share
    assert _rejected(c, st, st2, leaf, S) > 0
    assert R.judge(S, r.ref['S'], B, r.ref['A'])[1] > 0


@pytest.mark.parametrize('q', range(9))
def test_planted_one_element_one_percent_off(q):
    c, st, st2, r, B, leaf, S32 = _loose('partial-70x45-deg3')
    i = _typical(r.ref['S'], r.ref['A'], q)
    S = S32.copy()
    S[i, q] *= 1.01
    assert R.judge(S, r.ref['S'], B, r.ref['A'])[1] == 1
    assert _rejected(c, st, st2, leaf, S) > 0


def test_planted_conic_xx_and_yy_swapped():
    c, st, st2, r, B, leaf, S32 = _loose('partial-70x45-deg3')
    Sr, A = r.ref['S'], r.ref['A']
    differ = np.flatnonzero((A[:, 6] > 0) & (np.abs(Sr[:, 6] - Sr[:, 8]) >= 0.02 * (A[:, 6] + A[:, 8])))        # xx and yy are not nearly equal
    assert differ.size >= 5
    i = differ[np.argsort(np.abs(Sr[differ, 6] - Sr[differ, 8]))[differ.size // 2]]
    S = S32.copy()
    S[i, 6], S[i, 8] = S32[i, 8], S32[i, 6]
    assert _rejected(c, st, st2, leaf, S, leaves=('scale', 'rot', 'mean3D')) > 0


def test_planted_background_term_dropped():
    c, st, st2, r, B, leaf, S32 = _loose('partial-70x45-deg3')
    no_bg = R.BlendRef(r.st64, np.zeros(3)).sums(r.g)['S']
    assert _rejected(c, st, st2, leaf, S32 - (r.ref['S'] - no_bg)) > 100


def test_planted_clamped_sh_channel_with_its_unclamped_gradient():
    c, st, st2, r, B, leaf, S32 = _loose('clamp-sh-dc-x3')
    i, ch = np.argwhere((st.clamped != 0) & (r.ref['A'][:, :3] > 0))[0]
    flags = st.clamped.copy()
    flags[i, ch] = 0
    assert _rejected(c, st, st2, leaf, S32, leaves=('sh',), flags=flags) > 0


def test_planted_smallest_gaussian_zeroed():
    for name in ('partial-70x45-deg3', 'partial-113x71-2000-deg2'):
        c, st, st2, r, B, leaf, S32 = _loose(name)
        A = r.ref['A'][:, 6:9].sum(1)
        i = int(np.argmin(np.where(A > 0, A, np.inf)))
        print(f'{name}: smallest conic magnitude {A[i]:.3e}, largest {A.max():.3e}')
        S = S32.copy()
        S[i] = 0
        assert R.judge(S, r.ref['S'], B, r.ref['A'])[1] > 0 and _rejected(c, st, st2, leaf, S) > 0


def test_planted_scale_gradient_without_scale_modifier():
    c, st, st2, r, B, leaf, S32 = _loose('scale-modifier-0.7')
    got = C.oracle_leaves(c, st, st2, S32)
    assert R.judge(got['scale'], leaf.want['scale'], leaf.budget['scale'], leaf.A['scale'])[1:] == (0, 0)
    wrong = got['scale'] / np.float32(0.7)                           # the outer factor `mod` of dL_dscale left out
    assert R.judge(wrong, leaf.want['scale'], leaf.budget['scale'], leaf.A['scale'])[1] > 0.9 * (leaf.A['scale'] > 0).sum()


def test_planted_outside_pixels_of_a_partial_tile_counted():
    """A kernel without the `inside` mask: the pixel row below the image blends with the gradients (and the contributor counts) of the row above it."""
    c, st, st2, r, B, leaf, S32 = _loose('partial-70x45-deg3')
    taller = oracle.GSState()
    taller.__dict__.update(r.st64.__dict__)
    taller.H = c.h + 1
    ncon = st.n_contrib.reshape(c.h, c.w)
    taller.n_contrib = np.concatenate([ncon, ncon[-1:]]).reshape(-1)
    blend = R.BlendRef(taller, c.bg)
    assert not blend.ambiguous[-1].any()
    with_row = blend.sums(np.concatenate([r.g, r.g[:, -1:]], 1))['S']
    assert _rejected(c, st, st2, leaf, S32 + (with_row - r.ref['S'])) > 100


def test_judge_counts_non_finite_and_non_zero_elements():
    want, budget, A = np.array([1.0, 2.0, 0.0]), np.array([0.1, 0.1, 0.0]), np.array([1.0, 2.0, 0.0])
    assert R.judge(np.array([1.05, 2.0, 0.0]), want, budget, A) == (pytest.approx(0.5), 0, 0)
    assert R.judge(np.array([1.05, 2.0, -0.0]), want, budget, A)[2] == 0
    assert R.judge(np.array([1.2, 2.0, 1e-30]), want, budget, A)[1:] == (1, 1)
    assert R.judge(np.array([np.nan, 2.0, 0.0]), want, budget, A)[1] == 1
