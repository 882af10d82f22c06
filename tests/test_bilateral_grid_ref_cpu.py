"""CPU: the float64 restatement of the bilateral-grid slice (tests/bilateral_grid_ref.py) against torch.nn.functional.grid_sample on the interior cases, the
module's tensor formula against the restatement and its f32 evaluation against the error budget on every case, the g == 1 and out-of-range rules, the
total-variation term against its definition, the budget's size, and the host validation of the group-28 entry points (include/nerficg_hip.h)."""
import numpy as np
import pytest
import torch

from tests import bilateral_grid_ref as ref

ALL = tuple(ref.CASES) + ref.EXACT


def _close(got, want, what, tol=1e-12):
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=tol, atol=tol * max(float(np.abs(want).max()), 1e-300), err_msg=what)


def _formula(name, dtype):
    """tensor_formula on the case's inputs in its layout: out, affine, d_rgb as (H, W, .) numpy arrays, d_grids."""
    from nerficg_amd.bilateral_grid import slice as bg_slice
    grids, rgb, d_out = ref.inputs(name)
    _, _, idx, layout = ref.reference(name)
    g = torch.from_numpy(grids).to(dtype).requires_grad_(True)
    p = torch.from_numpy(ref.to_layout(rgb, layout)).to(dtype).requires_grad_(True)
    out, affine = bg_slice(g, p, idx, return_affine=True)              # CPU tensors: the module's fallback
    out.backward(torch.from_numpy(ref.to_layout(d_out, layout)).to(dtype))
    return (ref.from_layout(out.detach().numpy(), layout), affine.detach().numpy(), ref.from_layout(p.grad.numpy(), layout), g.grad.numpy())


@pytest.mark.parametrize('name', tuple(ref.CASES))
def test_the_drawn_cases_keep_the_margin(name):
    grids, rgb, d_out = ref.inputs(name)
    cell, g01 = ref.margins(grids.shape[2:], rgb)
    assert cell >= ref.MARGIN and g01 >= ref.MARGIN, (cell, g01)
    assert all(t.dtype == np.float32 for t in (grids, rgb, d_out))
    assert (d_out == 0).any() and (d_out > 0).any() and (d_out < 0).any()


@pytest.mark.parametrize('name', ref.INTERIOR)
def test_restatement_is_grid_sample_in_float64(name):
    """On interior inputs the definition is grid_sample(bilinear, align_corners=True, border) on (2u - 1, 2v - 1, 2g - 1): value and both gradients to 1e-12."""
    grids, rgb, d_out = ref.inputs(name)
    val, _, idx, _ = ref.reference(name)
    G = torch.from_numpy(grids).double().requires_grad_(True)
    p = torch.from_numpy(rgb).double().requires_grad_(True)
    H, W = rgb.shape[:2]
    u = ((torch.arange(W, dtype=torch.float64) + 0.5) / W)[None, :].expand(H, W)
    v = ((torch.arange(H, dtype=torch.float64) + 0.5) / H)[:, None].expand(H, W)
    g = (ref.CR * p[..., 0] + ref.CG * p[..., 1]) + ref.CB * p[..., 2]
    coords = torch.stack([2 * u - 1, 2 * v - 1, 2 * g - 1], -1)[None, None]                    # (1, 1, H, W, 3): x, y, z
    A = torch.nn.functional.grid_sample(G[idx][None], coords, mode='bilinear', align_corners=True, padding_mode='border')[0, :, 0].permute(1, 2, 0)
    M = A.reshape(H, W, 3, 4)
    out = (M[..., :3] * p[..., None, :]).sum(-1) + M[..., 3]
    out.backward(torch.from_numpy(d_out).double())
    _close(out.detach().numpy(), val['out'], 'out')
    _close(A.detach().numpy(), val['affine'], 'affine')
    _close(p.grad.numpy(), val['d_rgb'], 'd_rgb')
    _close(G.grad.numpy(), val['d_grids'], 'd_grids')


@pytest.mark.parametrize('name', tuple(ref.CASES))
def test_module_cpu_fallback_is_the_restatement_in_float64(name):
    """float64 CPU tensors take the tensor formula.  Its luminance constants are the doubles 0.299, 0.587, 0.114, the restatement's their f32 values like the
    kernel's: they differ by 4e-8 relatively, which (L - 1) and the vertex differences carry into the result -- 1e-6 of the tensor's scale is asked."""
    val = ref.reference(name)[0]
    for got, key in zip(_formula(name, torch.float64), ('out', 'affine', 'd_rgb', 'd_grids')):
        _close(got, val[key], key, tol=1e-6)


@pytest.mark.parametrize('name', ALL)
def test_tensor_formula_in_f32_within_budget(name):
    val, bud, _, _ = ref.reference(name)
    worst = {key: ref.assert_within_budget(got, val[key], bud[key], key) for got, key in zip(_formula(name, torch.float32), ('out', 'affine', 'd_rgb', 'd_grids'))}
    print(name, {k: round(v, 3) for k, v in worst.items()})


def test_white_is_g_one_in_f32_and_takes_the_last_cells_slope():
    assert ref.luminance_f32(np.ones(3, np.float32)) == 1.0 and (ref.CR + ref.CG) + ref.CB > 1.0        # f32 rounds to 1, float64 does not
    grids, rgb, d_out = ref.inputs('white')
    val = ref.reference('white')[0]
    L = grids.shape[2]
    G = grids[0].astype(np.float64)
    # every pixel: i_z = L - 2, f_z = 1 -- the output reads level L - 1 alone, the guidance gradient the slope of the last cell
    flat = ref.evaluate(np.repeat(G[None, :, L - 1:L], 1, axis=2), rgb, 0)
    np.testing.assert_allclose(val['out'], flat['out'], rtol=0, atol=1e-13)
    assert np.abs(val['d_rgb'] - np.einsum('hwr,hwrk->hwk', d_out.astype(np.float64), val['affine'].reshape(*rgb.shape[:2], 3, 4)[..., :3])).max() > 0.1
    _, _, d_rgb, _ = _formula('white', torch.float64)
    _close(d_rgb, val['d_rgb'], 'd_rgb at g == 1', tol=1e-6)


@pytest.mark.parametrize('name', ('above', 'below'))
def test_outside_the_range_the_guidance_carries_no_gradient(name):
    grids, rgb, d_out = ref.inputs(name)
    val = ref.reference(name)[0]
    lin = np.einsum('hwr,hwrk->hwk', d_out.astype(np.float64), val['affine'].reshape(*rgb.shape[:2], 3, 4)[..., :3])
    assert np.array_equal(val['d_rgb'], lin)
    assert np.abs(ref.reference('black')[0]['d_rgb'] - np.einsum('hwr,hwrk->hwk', ref.inputs('black')[2].astype(np.float64),
                                                                  ref.reference('black')[0]['affine'].reshape(4, 5, 3, 4)[..., :3])).max() > 0.1   # g == 0 is inside
    _, _, d_rgb, _ = _formula(name, torch.float64)
    _close(d_rgb, val['d_rgb'], 'd_rgb', tol=1e-6)


def test_pixel_centres_on_vertices_read_one_vertex_along_x_and_y():
    grids, rgb, _ = ref.inputs('vertices')
    val = ref.reference('vertices')[0]
    H, W = rgb.shape[:2]
    G = grids[0].astype(np.float64)
    for y in range(H):
        for x in range(W):
            vx, vy = (2 * x + 1), (2 * y + 1)                                                     # c_x = 8 (x + 0.5) / 4, c_y = 4 (y + 0.5) / 2
            cz = min(max(ref.CR * float(rgb[y, x, 0]), 0.0), 1.0) * 2
            iz = min(int(np.floor(cz)), 1)
            want = (1 - (cz - iz)) * G[:, iz, vy, vx] + (cz - iz) * G[:, iz + 1, vy, vx]
            np.testing.assert_allclose(val['affine'][y, x], want, rtol=0, atol=1e-13)


def test_one_vertex_is_a_global_affine():
    grids, rgb, _ = ref.inputs('affine')
    val = ref.reference('affine')[0]
    M = grids[0, :, 0, 0, 0].astype(np.float64).reshape(3, 4)
    np.testing.assert_allclose(val['out'], rgb.astype(np.float64) @ M[:, :3].T + M[:, 3], rtol=0, atol=1e-14)
    terms = np.abs(rgb.astype(np.float64)) @ np.abs(M[:, :3]).T + np.abs(M[:, 3])
    got = _formula('affine', torch.float32)[0]
    assert (np.abs(got - val['out']) <= 4 * ref.U * terms).all()      # one product and three additions at the most behind every term: its four roundings


def test_identity_grid_returns_the_input_and_has_a_grid_gradient():
    grids, rgb, d_out = ref.identity_case()
    val, bud = ref.evaluate(grids, rgb, 0, d_out), ref.budget(grids, rgb, 0, d_out)
    np.testing.assert_allclose(val['out'], rgb.astype(np.float64), rtol=0, atol=1e-15)
    assert np.abs(val['d_grids']).max() > 0.1
    from nerficg_amd.bilateral_grid import BilateralGrid
    bg = BilateralGrid(1, 4, 4, 4)
    assert np.array_equal(bg.grids.detach().numpy(), grids)
    p = torch.from_numpy(rgb).requires_grad_(True)
    out = bg(p, 0)
    out.backward(torch.from_numpy(d_out))
    ref.assert_within_budget(out.detach().numpy(), rgb, bud['out'], 'out')
    ref.assert_within_budget(bg.grids.grad.numpy(), val['d_grids'], bud['d_grids'], 'd_grids')
    ref.assert_within_budget(p.grad.numpy(), val['d_rgb'], bud['d_rgb'], 'd_rgb')


def test_other_grids_get_exactly_zero():
    val, _, idx, _ = ref.reference('lds')
    got = _formula('lds', torch.float32)[3]
    for n in range(got.shape[0]):
        assert (n == idx) == bool(got[n].any()) and (n == idx) == bool(val['d_grids'][n].any())


def test_ray_list_form_matches_the_image_form():
    from nerficg_amd.bilateral_grid import slice as bg_slice
    grids, rgb, _ = ref.inputs('cells')
    H, W = rgb.shape[:2]
    G, p = torch.from_numpy(grids).double(), torch.from_numpy(rgb).double()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    xy = torch.stack([(xs + 0.5) / W, (ys + 0.5) / H], -1).reshape(-1, 2).double()
    for n in range(grids.shape[0]):
        rays = bg_slice(G, p.reshape(-1, 3), torch.full((H * W,), n), xy=xy)
        assert torch.allclose(rays.reshape(H, W, 3), bg_slice(G, p, n), rtol=0, atol=1e-14)
    mixed = bg_slice(G, p.reshape(-1, 3), (torch.arange(H * W) % 2), xy=xy).reshape(H, W, 3)
    assert torch.equal(mixed.reshape(-1, 3)[1::2], bg_slice(G, p, 1).reshape(-1, 3)[1::2])


@pytest.mark.parametrize('shape', ref.TV_SHAPES)
def test_total_variation_against_its_definition(shape):
    from nerficg_amd.bilateral_grid import total_variation_loss
    G = ref.tv_inputs(shape).astype(np.float64)
    N, C, L, Gh, Gw = shape
    want = 0.0
    for axis, n in ((2, L), (3, Gh), (4, Gw)):
        if n > 1:
            d = np.diff(G, axis=axis)
            assert d.size == N * 12 * (n - 1) * (L * Gh * Gw // n)
            want += (d ** 2).sum() / (12 * (n - 1) * (L * Gh * Gw // n))
    want /= N
    assert abs(ref.tv(G) - want) <= 1e-15 * want
    t = torch.from_numpy(G).requires_grad_(True)
    tv = total_variation_loss(t)
    (tv * ref.UPSTREAM).backward()
    assert abs(tv.item() - want) <= 1e-14 * want
    _close(t.grad.numpy(), ref.tv_grad(G, ref.UPSTREAM), 'dTV/dG')
    eps, e = 1e-6, (1, 7, 0, 1, 3)                                                                # one element by central differences
    Gp, Gm = G.copy(), G.copy()
    Gp[e] += eps
    Gm[e] -= eps
    assert abs((ref.tv(Gp) - ref.tv(Gm)) / (2 * eps) - ref.tv_grad(G)[e]) <= 1e-8


def test_total_variation_of_a_constant_grid_is_exactly_zero():
    from nerficg_amd.bilateral_grid import total_variation_loss
    G = ref.tv_inputs(ref.TV_SHAPES[1], 'constant')
    assert ref.tv(G) == 0.0 and not ref.tv_grad(G).any()
    t = torch.from_numpy(G).requires_grad_(True)
    tv = total_variation_loss(t)
    tv.backward()
    assert tv.item() == 0.0 and not t.grad.numpy().any()


def test_gradcheck_of_the_tensor_formula():
    from nerficg_amd.bilateral_grid import tensor_formula
    grids, rgb, _ = ref.inputs('cell')
    G = torch.from_numpy(grids).double().requires_grad_(True)
    p = torch.from_numpy(ref.to_layout(rgb, 'chw')).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: tensor_formula(a, b, 0), (G, p), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_budget_maxima_stay_under_their_ceilings():
    got = ref.budget_maxima()
    print({k: f'{v:.3e}' for k, v in got.items()})
    for k, ceiling in ref.NAMED_CEILINGS.items():
        assert 0 < got[k] <= ceiling, (k, got[k])


def test_group_28_entry_points_validate_before_they_launch():
    """Null pointers, extents < 1, a host index outside [0, N) and zero strides return NRC_ERR_INVALID, an empty image NRC_OK -- on a machine without a GPU, so
    before any HIP call."""
    import ctypes
    from nerficg_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda **k: lib.nrc_bilagrid_slice_forward(*[k.get(a, d) for a, d in (('grids', P), ('N', 2), ('L', 2), ('Gh', 2), ('Gw', 2), ('rgb', P), ('H', 0), ('W', 0),
                                                                                ('ps', 1), ('cs', 1), ('idx', 0), ('idx_dev', None), ('out', P), ('affine', None),
                                                                                ('stream', None))])
    bwd = lambda **k: lib.nrc_bilagrid_slice_backward(*[k.get(a, d) for a, d in (('grids', P), ('N', 2), ('L', 2), ('Gh', 2), ('Gw', 2), ('rgb', P), ('d_out', P),
                                                                                 ('H', 0), ('W', 0), ('ps', 1), ('cs', 1), ('idx', 0), ('idx_dev', None), ('ws', P),
                                                                                 ('d_rgb', P), ('d_grids', None), ('stream', None))])
    assert fwd() == 0 and bwd() == 0                                                               # an empty image
    assert fwd(idx=1) == 0 and fwd(idx=2) == -1 and fwd(idx=-1) == -1 and fwd(idx=7, idx_dev=P) == 0   # a device index is not the host's to check
    for bad in (dict(grids=None), dict(rgb=None), dict(out=None), dict(N=0), dict(L=0), dict(Gh=0), dict(Gw=-1), dict(H=-1), dict(W=-1), dict(ps=0), dict(cs=0)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(grids=None), dict(rgb=None), dict(d_out=None), dict(d_rgb=None), dict(N=0), dict(L=0), dict(Gh=0), dict(Gw=0), dict(H=-1), dict(ps=0),
                dict(cs=0), dict(idx=2), dict(d_grids=P, ws=None, H=4, W=4)):
        assert bwd(**bad) == -1, bad
    assert lib.nrc_bilagrid_tv_forward(None, 1, 2, 2, 2, P, P, None) == -1 and lib.nrc_bilagrid_tv_forward(P, 1, 2, 2, 2, None, P, None) == -1
    assert lib.nrc_bilagrid_tv_forward(P, 1, 2, 2, 2, P, None, None) == -1 and lib.nrc_bilagrid_tv_forward(P, 0, 2, 2, 2, P, P, None) == -1
    assert lib.nrc_bilagrid_tv_backward(None, 1, 2, 2, 2, None, P, None) == -1 and lib.nrc_bilagrid_tv_backward(P, 1, 2, 2, 2, None, None, None) == -1
    assert lib.nrc_bilagrid_tv_backward(P, 1, 0, 2, 2, None, P, None) == -1
    # the workspace: the TV partials alone for an empty image; a partial window per 32 x 8 tile where the window fits LDS (3 x 2 x 8 x 12 floats at 1297 x 840)
    assert lib.nrc_bilagrid_ws_floats(0, 8, 16, 16, 8, 8) == -1 and lib.nrc_bilagrid_ws_floats(1, 8, 16, 16, -1, 8) == -1
    assert lib.nrc_bilagrid_ws_floats(200, 8, 16, 16, 0, 0) == 6144
    assert lib.nrc_bilagrid_ws_floats(200, 8, 16, 16, 840, 1297) == 41 * 105 * 3 * 2 * 8 * 12              # cells of 86.5 x 56 pixels: a tile row never straddles a cell border
    assert lib.nrc_bilagrid_ws_floats(1, 8, 16, 16, 37, 70) == 6144                                # the direct path keeps no partials
    assert lib.nrc_bilagrid_ws_floats(3, 8, 4, 4, 96, 200) == 7 * 12 * 3 * 2 * 8 * 12


def test_module_rejects_what_it_cannot_slice():
    from nerficg_amd.bilateral_grid import slice as bg_slice
    with pytest.raises(RuntimeError, match=r'\(3, H, W\) or \(H, W, 3\)'):
        bg_slice(torch.zeros(1, 12, 2, 2, 2), torch.zeros(4, 5, 4), 0)
    with pytest.raises(RuntimeError, match='N, 12, L, Gh, Gw'):
        bg_slice(torch.zeros(1, 9, 2, 2, 2), torch.zeros(3, 5, 4), 0)
