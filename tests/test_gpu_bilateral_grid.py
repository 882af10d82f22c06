"""GPU: the fused bilateral-grid slice, its two gradients and the total-variation term (nerficg_amd.bilateral_grid, nerficg_amd/csrc/bilateral_grid.hip, C ABI
group 28) against the float64 restatement and the per-element f32 budget of tests/bilateral_grid_ref.py (pinned to grid_sample in
tests/test_bilateral_grid_ref_cpu.py), plus bit-for-bit reproducibility, host and device grid index, the way through the rasterizer and a captured graph."""
import math

import numpy as np
import pytest
import torch

from tests import bilateral_grid_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ALL = tuple(ref.CASES) + ref.EXACT


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _run(name, device_idx=False, rgb_grad=True, grids_grad=True):
    """slice(return_affine=True) and its backward on the case's inputs in the case's layout: (out, affine, d_rgb, d_grids) as numpy, (H, W, .) images."""
    from nerficg_amd.bilateral_grid import slice as bg_slice
    grids, rgb, d_out = ref.inputs(name)
    _, _, idx, layout = ref.reference(name)
    g, p = T(grids).requires_grad_(grids_grad), T(ref.to_layout(rgb, layout)).requires_grad_(rgb_grad)
    out, affine = bg_slice(g, p, torch.tensor([idx], dtype=torch.int32, device=DEV) if device_idx else idx, return_affine=True)
    assert type(out.grad_fn).__name__ == '_SliceBackward'                       # the kernels ran, as one node
    out.backward(T(ref.to_layout(d_out, layout)))
    back = lambda t: None if t.grad is None else t.grad.cpu().numpy()
    d_rgb = back(p)
    return (ref.from_layout(out.detach().cpu().numpy(), layout), affine.cpu().numpy(), None if d_rgb is None else ref.from_layout(d_rgb, layout), back(g))


@pytest.mark.parametrize('name', ALL)
def test_output_matrices_and_every_gradient_element_within_budget(name):
    grids, rgb, _ = ref.inputs(name)
    if name in ref.CASES:
        cell, g01 = ref.margins(grids.shape[2:], rgb)
        assert cell >= ref.MARGIN and g01 >= ref.MARGIN                         # no kink within reach of an f32 rounding: every element is compared
    val, bud, idx, _ = ref.reference(name)
    got = _run(name)
    worst = {key: ref.assert_within_budget(g, val[key], bud[key], key) for g, key in zip(got, ('out', 'affine', 'd_rgb', 'd_grids'))}
    for n in range(grids.shape[0]):
        if n != idx:
            assert not got[3][n].any(), f'slice {n} of d_grids'                 # every other grid: exactly zero
    assert got[3][idx].any()
    print(name, {k: round(v, 3) for k, v in worst.items()})
    only_rgb, only_grids = _run(name, grids_grad=False), _run(name, rgb_grad=False)
    assert only_rgb[3] is None and only_grids[2] is None
    assert np.array_equal(only_rgb[2], got[2]) and np.array_equal(only_grids[3], got[3]) and np.array_equal(only_rgb[0], got[0])


def test_one_vertex_is_a_global_affine_within_its_four_roundings():
    grids, rgb, _ = ref.inputs('affine')
    M = grids[0, :, 0, 0, 0].astype(np.float64).reshape(3, 4)
    p = rgb.astype(np.float64)
    terms = np.abs(p) @ np.abs(M[:, :3]).T + np.abs(M[:, 3])
    assert (np.abs(_run('affine')[0] - (p @ M[:, :3].T + M[:, 3])) <= 4 * ref.U * terms).all()


def test_identity_grid_returns_the_input_and_has_a_grid_gradient():
    from nerficg_amd.bilateral_grid import BilateralGrid
    grids, rgb, d_out = ref.identity_case()
    val, bud = ref.evaluate(grids, rgb, 0, d_out), ref.budget(grids, rgb, 0, d_out)
    bg = BilateralGrid(1, 4, 4, 4).to(DEV)
    assert np.array_equal(bg.grids.detach().cpu().numpy(), grids)
    p = T(rgb).requires_grad_(True)
    out = bg(p, 0)
    out.backward(T(d_out))
    ref.assert_within_budget(out.detach().cpu().numpy(), rgb, bud['out'], 'out')
    ref.assert_within_budget(bg.grids.grad.cpu().numpy(), val['d_grids'], bud['d_grids'], 'd_grids')
    ref.assert_within_budget(p.grad.cpu().numpy(), val['d_rgb'], bud['d_rgb'], 'd_rgb')
    assert np.abs(bg.grids.grad.cpu().numpy()).max() > 0.1


def test_exact_rules_at_the_ends_of_the_luminance_range():
    """White takes the last cell's slope, (2, 2, 2) and (-1, -1, -1) have no guidance gradient: d_rgb is the linear part alone, within ITS three roundings."""
    for name in ('above', 'below'):
        _, _, d_out = ref.inputs(name)
        out, affine, d_rgb, _ = _run(name)
        A = affine.astype(np.float64).reshape(*d_out.shape[:2], 3, 4)[..., :3]
        d = d_out.astype(np.float64)
        lin, mag = np.einsum('hwr,hwrk->hwk', d, A), np.einsum('hwr,hwrk->hwk', np.abs(d), np.abs(A))
        assert (np.abs(d_rgb - lin) <= 3 * ref.U * mag).all(), name
    val = ref.reference('white')[0]
    _, affine, d_rgb, _ = _run('white')
    d = ref.inputs('white')[2].astype(np.float64)
    lin = np.einsum('hwr,hwrk->hwk', d, affine.astype(np.float64).reshape(*d.shape[:2], 3, 4)[..., :3])
    assert np.abs(d_rgb - lin).max() > 0.1 and np.abs(val['d_rgb'] - lin).max() > 0.1                 # the guidance part is there


@pytest.mark.parametrize('name', ('lds', 'many', 'direct'))
def test_two_calls_give_the_same_bits(name):
    a, b = _run(name), _run(name)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    from nerficg_amd.bilateral_grid import total_variation_loss
    G = T(ref.tv_inputs(ref.TV_SHAPES[0]))
    res = []
    for _ in range(2):
        g = G.clone().requires_grad_(True)
        tv = total_variation_loss(g)
        tv.backward()
        res.append((tv.item(), g.grad.cpu().numpy()))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize('name', ('lds', 'direct', 'cells'))
def test_host_index_and_device_index_give_the_same_bits(name):
    for x, y in zip(_run(name), _run(name, device_idx=True)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('shape', ref.TV_SHAPES)
def test_total_variation_and_its_gradient_within_budget(shape):
    from nerficg_amd.bilateral_grid import total_variation_loss
    G = ref.tv_inputs(shape)
    g = T(G).requires_grad_(True)
    tv = total_variation_loss(g)
    assert type(tv.grad_fn).__name__ == '_TotalVariationBackward'
    (tv * ref.UPSTREAM).backward()
    e_tv, e_grad = ref.tv_budget(G, ref.UPSTREAM)
    worst = ref.assert_within_budget(tv.item(), ref.tv(G), e_tv, 'TV'), ref.assert_within_budget(g.grad.cpu().numpy(), ref.tv_grad(G, ref.UPSTREAM), e_grad, 'dTV/dG')
    print(shape, [round(w, 3) for w in worst])


def test_total_variation_of_a_constant_grid_is_exactly_zero():
    from nerficg_amd.bilateral_grid import total_variation_loss
    for shape in ref.TV_SHAPES:
        g = T(ref.tv_inputs(shape, 'constant')).requires_grad_(True)
        tv = total_variation_loss(g)
        tv.backward()
        assert tv.item() == 0.0 and not g.grad.cpu().numpy().any()


def test_through_the_rasterizer():
    """render -> bg(out['rgb'], i) -> loss: the gradient that reaches the rendered image is the reference's, evaluated on the rendered image, within its budget."""
    from nerficg_amd.bilateral_grid import BilateralGrid
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sc = scenes.gs_random_scene(300, seed=11, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=3)
    cam = scenes.gs_camera(48, 40, scenes.orbit_pose(0.5, 0.3, 3.0))
    settings = GaussianRasterizationSettings(
        image_height=cam['height'], image_width=cam['width'], tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=T(np.asarray([0.2, 0.4, 0.1], np.float32)),
        scale_modifier=1.0, viewmatrix=T(cam['viewmatrix']), projmatrix=T(cam['projmatrix']), sh_degree=sc['sh_degree'], campos=T(cam['campos']),
        prefiltered=False, debug=False)
    t = {k: T(v).requires_grad_(True) for k, v in sc.items() if k != 'sh_degree'}
    t['means2D'] = torch.zeros_like(t['means3D'], requires_grad=True)
    image, _ = GaussianRasterizer(settings)(means3D=t['means3D'], means2D=t['means2D'], opacities=t['opacities'][:, None], shs=t['shs'], scales=t['scales'],
                                            rotations=t['rotations'])
    image.retain_grad()
    grids = ref.draw(2, (8, 4, 4), 40, 48, seed=21)[0]
    bg = BilateralGrid(2, 4, 4, 8).to(DEV)
    with torch.no_grad():
        bg.grids.copy_(T(grids))
    target = T(np.random.default_rng(5).random((3, 40, 48)))
    out = bg(image, 1)
    ((out - target) ** 2).sum().backward()
    assert t['means3D'].grad is not None and float(t['shs'].grad.abs().max()) > 0
    rendered = image.detach().cpu().numpy().transpose(1, 2, 0)
    cell, g01 = ref.margins((8, 4, 4), rendered)
    assert cell >= ref.MARGIN and g01 >= ref.MARGIN, 'the rendered image has a pixel on a kink: choose another scene'
    d_out = (2 * (out.detach() - target)).cpu().numpy().transpose(1, 2, 0)
    val, bud = ref.evaluate(grids, rendered, 1, d_out), ref.budget(grids, rendered, 1, d_out)
    ref.assert_within_budget(out.detach().cpu().numpy().transpose(1, 2, 0), val['out'], bud['out'], 'out')
    ref.assert_within_budget(image.grad.cpu().numpy().transpose(1, 2, 0), val['d_rgb'], bud['d_rgb'], "out['rgb'].grad")
    ref.assert_within_budget(bg.grids.grad.cpu().numpy(), val['d_grids'], bud['d_grids'], 'd_grids')


def test_captured_graph_replays_on_changed_inputs_and_a_changed_device_index():
    """Slice forward + backward + TV captured once as a linear graph, replayed on other values in the static buffers and another grid index on the device:
    the same bits as the eager calls on those values."""
    from nerficg_amd.bilateral_grid import slice as bg_slice, total_variation_loss
    n, shape, H, W, idx, layout = ref.CASES['lds']
    first, second = ref.draw(n, shape, H, W, seed=8), ref.inputs('lds')
    static = [T(first[0]).requires_grad_(True), T(first[1]).requires_grad_(True)]
    d_out, index = T(first[2]), torch.tensor([0], dtype=torch.int32, device=DEV)

    def step():
        out = bg_slice(static[0], static[1], index)
        tv = total_variation_loss(static[0])
        return (out, tv) + torch.autograd.grad([out, tv], static, [d_out, torch.full_like(tv, ref.UPSTREAM)])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        static[0].copy_(T(second[0])), static[1].copy_(T(second[1])), d_out.copy_(T(second[2])), index.fill_(idx)
    graph.replay()
    torch.cuda.synchronize()
    g, p = T(second[0]).requires_grad_(True), T(second[1]).requires_grad_(True)
    out = bg_slice(g, p, idx)
    tv = total_variation_loss(g)
    want = (out, tv) + torch.autograd.grad([out, tv], [g, p], [T(second[2]), torch.full_like(tv, ref.UPSTREAM)])
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    val, bud, _, _ = ref.reference('lds')
    ref.assert_within_budget(outs[0].detach().cpu().numpy(), val['out'], bud['out'], 'out after the replay')
