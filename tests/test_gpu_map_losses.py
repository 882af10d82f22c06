"""GPU: the fused depth-smoothness / alpha-entropy losses (nerficg_amd.map_losses, nerficg_amd/csrc/map_losses.hip, C ABI group 15) against the float64
restatement and the per-element f32 budget of tests/map_losses_ref.py (pinned to the reference's functions in tests/test_map_losses_cpu.py), plus
determinism, the decomposition in ctx.terms, the unchanged default of training_loss, the whole way through the rasterizer, and a captured graph."""
import math

import numpy as np
import pytest
import torch

from tests import map_losses_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _run(shape, normalize, symmetrical, weights, image_grad=True, upstream=ref.UPSTREAM):
    """map_regularizer on the case's inputs; (loss, terms[4], g_depth, g_alpha, g_image) as numpy, missing gradients as None."""
    from nerficg_amd.map_losses import map_regularizer
    depth, alpha, image = (T(t) for t in ref.inputs(shape))
    depth.requires_grad_(True), alpha.requires_grad_(True), image.requires_grad_(image_grad)
    loss = map_regularizer(depth, alpha, image, weights[0], weights[1], normalize=normalize, symmetrical=symmetrical)
    terms = loss.grad_fn.terms
    (loss * upstream).backward()
    grads = [None if t.grad is None else t.grad.cpu().numpy() for t in (depth, alpha, image)]
    return loss.item(), terms.cpu().numpy(), grads


@pytest.mark.parametrize('name,shape,normalize,symmetrical,weights', ref.all_cases())
def test_value_terms_and_every_gradient_element_within_budget(name, shape, normalize, symmetrical, weights):
    if shape != 'ties':
        lap, dimg = ref.margins(*ref.inputs(shape))
        assert lap >= ref.MARGIN and dimg >= ref.MARGIN                     # no kink within reach of an f32 rounding: every element is compared
    val, bud = ref.reference(shape, normalize, symmetrical, weights, ref.UPSTREAM)
    smooth, entropy = weights[0] != 0, weights[1] != 0
    for image_grad in (True, False):
        loss, terms, (gd, ga, gi) = _run(shape, normalize, symmetrical, weights, image_grad)
        worst = {'loss': ref.assert_within_budget(loss, val['loss'], bud['loss'], 'loss')}
        assert terms[0] == np.float32(loss)
        for k, key in ((1, 'S_x'), (2, 'S_y'), (3, 'E')):                    # ctx.terms: the separately computed terms (zero for a term that is switched off)
            worst[key] = ref.assert_within_budget(terms[k], val[key], bud[key], key)
        assert (gd is not None) == smooth and (ga is not None) == (entropy or (smooth and normalize)) and (gi is not None) == (smooth and image_grad)
        for got, key in ((gd, 'g_depth'), (ga, 'g_alpha'), (gi, 'g_image')):
            if got is not None:
                worst[key] = ref.assert_within_budget(got, val[key], bud[key], key)
            elif key != 'g_image' or image_grad:
                assert not val[key].any(), key                               # no gradient handed out: there is none
        print(name, f'image_grad={image_grad}', {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize('shape', [(2, 4, 33, 65), ref.MANY_WORKGROUPS])
def test_two_calls_give_the_same_bits(shape):
    a = _run(shape, True, True, ref.WEIGHTS[2])
    b = _run(shape, True, True, ref.WEIGHTS[2])
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


def test_reference_signatures_run_the_kernels():
    from nerficg_amd.map_losses import background_entropy, depth_smoothness_loss
    shape = (2, 4, 33, 65)
    depth, alpha, image = (T(t) for t in ref.inputs(shape))
    val, bud = ref.reference(shape, False, True, ref.WEIGHTS[2])
    s = depth_smoothness_loss(depth[:, None].requires_grad_(True), image)
    assert s.grad_fn is not None and hasattr(s.grad_fn, 'terms') and s.dim() == 0
    assert abs(s.item() - (val['S_x'] + val['S_y'])) <= bud['S_x'] + bud['S_y'] + ref.U * abs(s.item())
    e = background_entropy(alpha.reshape(2, 1, 33, 65), symmetrical=True)
    assert abs(e.item() - val['E']) <= bud['E']
    with pytest.raises(RuntimeError, match='at least 3'):
        depth_smoothness_loss(depth[:, None, :2], image[:, :, :2])


def test_training_loss_without_the_new_keywords_is_the_photometric_loss_bit_for_bit():
    from nerficg_amd.fused_ssim import photometric_loss
    from nerficg_amd.gaussian_splatting import training_loss
    rng = np.random.default_rng(3)
    image, target = T(rng.random((3, 40, 48))), T(rng.random((3, 40, 48)))
    a, b = image.clone().requires_grad_(True), image.clone().requires_grad_(True)
    la = training_loss(a, target)
    lb = photometric_loss(b[None], target[None], 0.8, 0.2)
    assert type(la.grad_fn).__name__ == type(lb.grad_fn).__name__            # the same single node, nothing behind it
    la.backward(), lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b.grad)


def _render(sc, cam):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    settings = GaussianRasterizationSettings(
        image_height=cam['height'], image_width=cam['width'], tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=T(np.asarray([0.2, 0.4, 0.1], np.float32)),
        scale_modifier=1.0, viewmatrix=T(cam['viewmatrix']), projmatrix=T(cam['projmatrix']), sh_degree=sc['sh_degree'], campos=T(cam['campos']),
        prefiltered=False, debug=False)
    t = {k: T(v).requires_grad_(True) for k, v in sc.items() if k != 'sh_degree'}
    t['means2D'] = torch.zeros_like(t['means3D'], requires_grad=True)
    image, radii, depth_sum, alpha = GaussianRasterizer(settings)(means3D=t['means3D'], means2D=t['means2D'], opacities=t['opacities'][:, None], shs=t['shs'],
                                                                  scales=t['scales'], rotations=t['rotations'], return_depth_alpha=True)
    return t, image, depth_sum, alpha


def test_end_to_end_through_the_rasterizer_matches_the_tensor_formula_loss():
    """render (return_depth_alpha=True) -> training_loss(depth=, alpha=, lambda_smooth=0.1, lambda_entropy=0.01) against the same rasterizer call under the
    tensor-formula loss; parameter gradients within the rasterizer gradient tolerance of tests/test_gpu_gs_depth_alpha.py (max error <= 2e-3 scale + 1e-6,
    mean error <= 1e-4 scale + 1e-7, scale = the reference tensor's largest magnitude)."""
    from nerficg_amd.fused_ssim import photometric_loss
    from nerficg_amd.gaussian_splatting import training_loss
    from nerficg_amd.map_losses import tensor_formula
    sc = scenes.gs_random_scene(300, seed=11, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=3)
    cam = scenes.gs_camera(48, 40, scenes.orbit_pose(0.5, 0.3, 3.0))
    target = T(np.random.default_rng(5).random((3, 40, 48)))
    leaves, image, depth_sum, alpha = _render(sc, cam)
    assert depth_sum.shape == alpha.shape == (40, 48) and float(alpha.detach().max()) > 0.5
    loss = training_loss(image, target, depth=depth_sum, alpha=alpha, lambda_smooth=0.1, lambda_entropy=0.01)
    loss.backward()
    want_leaves, image2, depth2, alpha2 = _render(sc, cam)
    want = photometric_loss(image2[None], target[None], 0.8, 0.2) + tensor_formula(depth2[None], alpha2[None], image2[None], 0.1, 0.01, True, False)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    for name in ('means3D', 'means2D', 'opacities', 'scales', 'rotations', 'shs'):
        g, r = leaves[name].grad.cpu().numpy(), want_leaves[name].grad.cpu().numpy()
        scale = np.abs(r).max()
        assert scale > 0 and np.isfinite(g).all(), name
        err = np.abs(g - r)
        print(f'{name}: max error {err.max():.3e} (bound {2e-3 * scale + 1e-6:.3e})  mean error {err.mean():.3e} (bound {1e-4 * scale + 1e-7:.3e})')
        assert err.max() <= 2e-3 * scale + 1e-6 and err.mean() <= 1e-4 * scale + 1e-7, name


def test_captured_graph_replays_on_changed_inputs():
    """Forward and backward captured once (a capture refuses a synchronisation or a host read), replayed once on other values in the static buffers: the
    same bits as the eager call on those values."""
    from nerficg_amd.map_losses import map_regularizer
    shape = (2, 4, 33, 65)
    first, second = ref.draw(shape, seed=8), ref.inputs(shape)
    static = [T(t).requires_grad_(True) for t in first]

    def step():
        loss = map_regularizer(*static, 0.1, 0.01, normalize=True, symmetrical=True)
        return (loss, loss.grad_fn.terms) + torch.autograd.grad(loss * ref.UPSTREAM, static)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        for s, t in zip(static, second):
            s.copy_(T(t))
    graph.replay()
    torch.cuda.synchronize()
    loss, terms, grads = _run(shape, True, True, ref.WEIGHTS[2])
    assert outs[0].item() == loss and np.array_equal(outs[1].cpu().numpy(), terms)
    for got, want in zip(outs[2:], grads):
        assert np.array_equal(got.cpu().numpy(), want)
