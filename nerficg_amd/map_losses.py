"""nerficg_amd.map_losses -- the regularisers that consume the 3DGS rasterizer's depth and alpha maps, as one autograd node over three launches.

depth_smoothness_loss(depth, image) and background_entropy(input, symmetrical=False) have the signatures and the values of the reference's functions
(src/Optim/Losses/DepthSmoothness.py:31-43, src/Optim/Losses/BackgroundEntropy.py:6-8); map_regularizer is both terms and the depth / (alpha + 1e-6)
normalisation in front of them (InstantNGP/Renderer.py:82) in one node.  Kernels: nerficg_amd/csrc/map_losses.hip through the C ABI
(include/nerficg_hip.h group 15).  CPU tensors and dtypes other than f32 take the tensor formula (`tensor_formula`), which is also what the kernels are
tested against.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ['depth_smoothness_loss', 'background_entropy', 'map_regularizer', 'tensor_formula']

EPS = 1e-6


def _second_difference(t: torch.Tensor, dim: int) -> torch.Tensor:
    n = t.shape[dim] - 2
    return t.narrow(dim, 0, n) + t.narrow(dim, 2, n) - 2 * t.narrow(dim, 1, n)


def _edge_weight(image: torch.Tensor, dim: int) -> torch.Tensor:
    """exp(-mean_c |I[x] - I[x-1]|) at the centres 1 .. n-2 along `dim`."""
    n = image.shape[dim] - 2
    step = image.narrow(dim, 1, n) - image.narrow(dim, 0, n)
    return torch.exp(-step.abs().mean(dim=1, keepdim=True))


def _smoothness_formula(depth: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    """The value of DepthSmoothness.py:31-43 on depth (B, 1, H, W) and image (B, C, H, W): S_x + S_y."""
    s_x, s_y = ((_second_difference(depth, dim) * _edge_weight(image, dim)).abs().mean() for dim in (3, 2))
    return s_x + s_y


def _entropy_formula(alpha: torch.Tensor, symmetrical: bool) -> torch.Tensor:
    """The value of BackgroundEntropy.py:6-8."""
    a = alpha.clamp(1e-6, 1.0 - 1e-6)
    h = -(a * a.log())
    if symmetrical:
        b = 1 - a
        h = h - b * b.log()
    return h.mean()


def tensor_formula(depth, alpha, image, lambda_smooth: float, lambda_entropy: float, normalize: bool = True, symmetrical: bool = False) -> torch.Tensor:
    """map_regularizer as tensor operations (any device, any floating dtype): depth, alpha (B, H, W), image (B, C, H, W)."""
    loss = None
    if lambda_smooth != 0:
        d = depth / (alpha + EPS) if normalize else depth
        loss = lambda_smooth * _smoothness_formula(d[:, None], image)
    if lambda_entropy != 0:
        e = lambda_entropy * _entropy_formula(alpha, symmetrical)
        loss = e if loss is None else loss + e
    if loss is None:
        raise RuntimeError('map_regularizer: lambda_smooth and lambda_entropy are both zero')
    return loss


class _MapRegularizer(torch.autograd.Function):
    """lambda_smooth (S_x + S_y) + lambda_entropy E as ONE node: stencil + reduction forward, one stencil backward (nrc_map_losses_*).  The upstream gradient of
    the loss value stays on the device.  Nothing is read back and every size comes from the shapes, so the node is capturable."""

    @staticmethod
    def forward(ctx, depth, alpha, image, lambda_smooth, lambda_entropy, normalize, symmetrical):
        lib = _lib.load()
        ref = depth if depth is not None else alpha
        b, h, w = ref.shape
        c = image.shape[1] if image is not None else 1
        ws = torch.empty(int(lib.nrc_map_losses_ws_floats(b, h, w)), dtype=torch.float32, device=ref.device)
        loss4 = torch.empty(4, dtype=torch.float32, device=ref.device)
        _lib.check(lib.nrc_map_losses_forward(_lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(image), b, c, h, w, int(normalize), lambda_smooth, lambda_entropy,
                                              int(symmetrical), _lib.ptr(ws), _lib.ptr(loss4), _lib.stream_of(ref)), 'map_losses_forward')
        ctx.save_for_backward(*(t.detach() if t is not None else None for t in (depth, alpha, image)))
        ctx.args = (b, c, h, w, int(normalize), lambda_smooth, lambda_entropy, int(symmetrical))
        ctx.terms = loss4      # {loss, S_x, S_y, E} on the device, for logging without another pass
        return loss4[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        depth, alpha, image = ctx.saved_tensors
        b, c, h, w, normalize, lambda_smooth, lambda_entropy, symmetrical = ctx.args
        lib = _lib.load()
        smooth = lambda_smooth != 0.0
        want_d = smooth and ctx.needs_input_grad[0]
        want_a = alpha is not None and ctx.needs_input_grad[1] and ((smooth and normalize) or lambda_entropy != 0.0)
        want_i = smooth and ctx.needs_input_grad[2]
        g_d = torch.empty_like(depth) if want_d else None
        g_a = torch.empty_like(alpha) if want_a else None
        g_i = torch.empty_like(image) if want_i else None
        if want_d or want_a or want_i:
            ref = depth if depth is not None else alpha
            g = grad_loss.to(torch.float32).reshape(1).contiguous()
            _lib.check(lib.nrc_map_losses_backward(_lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(image), b, c, h, w, normalize, lambda_smooth, lambda_entropy,
                                                   symmetrical, _lib.ptr(g), _lib.ptr(g_d), _lib.ptr(g_a), _lib.ptr(g_i), _lib.stream_of(ref)),
                       'map_losses_backward')
        return g_d, g_a, g_i, None, None, None, None


def _maps(t, name):
    """(H, W) / (B, H, W) / (B, 1, H, W) -> (B, H, W), as a view."""
    if t is None:
        return None
    if t.dim() == 2:
        return t[None]
    if t.dim() == 4 and t.shape[1] == 1:
        return t[:, 0]
    if t.dim() != 3:
        raise RuntimeError(f'map_regularizer: {name} must be (H, W), (B, H, W) or (B, 1, H, W), got {tuple(t.shape)}')
    return t


def map_regularizer(depth, alpha, image, lambda_smooth: float, lambda_entropy: float, normalize: bool = True, symmetrical: bool = False) -> torch.Tensor:
    """lambda_smooth * depth_smoothness_loss(d, image) + lambda_entropy * background_entropy(alpha, symmetrical) with d = depth / (alpha + 1e-6) when
    `normalize` (depth is then the rasterizer's ACCUMULATED depth sum w z, as `return_depth_alpha=True` hands it out) or d = depth.  One autograd node with
    gradients for depth, alpha and image (the image's is skipped when it needs none); `.grad_fn.terms` holds {loss, S_x, S_y, E} on the device.
    depth, alpha: (H, W), (B, H, W) or (B, 1, H, W); image: (C, H, W) or (B, C, H, W), 1 <= C <= 4.  A weight of zero drops that term and its inputs
    (depth and image may be None with lambda_smooth == 0, alpha with lambda_entropy == 0 and normalize=False).  H, W >= 3."""
    lambda_smooth, lambda_entropy = float(lambda_smooth), float(lambda_entropy)
    if lambda_smooth == 0.0 and lambda_entropy == 0.0:
        raise RuntimeError('map_regularizer: lambda_smooth and lambda_entropy are both zero')
    depth, alpha = _maps(depth, 'depth'), _maps(alpha, 'alpha')
    if image is not None and image.dim() == 3:
        image = image[None]
    if lambda_smooth == 0.0:
        depth = image = None
    elif depth is None or image is None:
        raise RuntimeError('map_regularizer: lambda_smooth != 0 needs depth and image')
    if lambda_entropy == 0.0 and not (normalize and lambda_smooth != 0.0):
        alpha = None
    elif alpha is None:
        raise RuntimeError('map_regularizer: alpha is needed (lambda_entropy != 0, or normalize=True)')
    given = [t for t in (depth, alpha, image) if t is not None]
    ref = given[0]
    if ref.shape[-2] < 3 or ref.shape[-1] < 3:
        raise RuntimeError(f'map_regularizer: maps of {ref.shape[-2]} x {ref.shape[-1]} pixels -- H and W must be at least 3 (the means over an empty set are NaN)')
    if depth is not None and (image.dim() != 4 or image.shape[0] != depth.shape[0] or image.shape[2:] != depth.shape[1:] or not 1 <= image.shape[1] <= 4):
        raise RuntimeError(f'map_regularizer: image {tuple(image.shape)} does not belong to depth {tuple(depth.shape)} (B, C <= 4, H, W)')
    if depth is not None and alpha is not None and alpha.shape != depth.shape:
        raise RuntimeError(f'map_regularizer: alpha {tuple(alpha.shape)} and depth {tuple(depth.shape)} differ in shape')
    if not all(t.is_cuda and t.dtype == torch.float32 for t in given):
        return tensor_formula(depth, alpha, image, lambda_smooth, lambda_entropy, normalize, symmetrical)
    return _MapRegularizer.apply(*(t.contiguous() if t is not None else None for t in (depth, alpha, image)), lambda_smooth, lambda_entropy, bool(normalize),
                                 bool(symmetrical))


def depth_smoothness_loss(depth: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    """DepthSmoothness.py:31-43: depth (B, 1, H, W), image (B, C, H, W) -> scalar."""
    if depth.dim() != 4 or depth.shape[1] != 1 or image.dim() != 4:
        raise RuntimeError('depth_smoothness_loss: depth must be (B, 1, H, W) and image (B, C, H, W)')
    if not (depth.is_cuda and image.is_cuda and depth.dtype == image.dtype == torch.float32 and 1 <= image.shape[1] <= 4):
        return _smoothness_formula(depth, image)
    return map_regularizer(depth, None, image, 1.0, 0.0, normalize=False)


def background_entropy(input: torch.Tensor, symmetrical: bool = False) -> torch.Tensor:
    """BackgroundEntropy.py:6-8: any shape -> scalar.  The kernels take maps: the last two dimensions are the map (both >= 3), the others the batch; any other shape
    takes the tensor formula."""
    if not (input.is_cuda and input.dtype == torch.float32 and input.dim() >= 2 and input.shape[-1] >= 3 and input.shape[-2] >= 3 and 1 <= input.numel() // (input.shape[-1] * input.shape[-2]) <= 65535):
        return _entropy_formula(input, symmetrical)
    return map_regularizer(None, input.reshape(-1, input.shape[-2], input.shape[-1]), None, 0.0, 1.0, normalize=False, symmetrical=symmetrical)
