"""nerficg_amd.bilateral_grid -- per-image colour correction by a bilateral grid of 3 x 4 colour transforms ("Bilateral Guided Radiance Field Processing",
Wang et al., SIGGRAPH 2024; gsplat: use_bilateral_grid): every training image owns a small (12, L, Gh, Gw) grid, sliced per pixel by position and luminance and
applied to the rendered image before the loss, with a total-variation term on the grids.  include/nerficg_hip.h group 28 states the definition.

Kernels: nerficg_amd/csrc/bilateral_grid.hip through the C ABI.  Each of the two operations (`slice`, `total_variation_loss`) is ONE autograd node; nothing
is read back and every size comes from the shapes, so both are capturable, and the grid index may be a device int32 that a captured iteration changes.  The
grid gradient is summed in a fixed order: the same input gives the same bits.  CPU tensors, dtypes other than f32 and the ray-list form (`xy` with per-ray
`idx`) take the tensor formula (`tensor_formula`), which is also what the kernels are tested against.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ['BilateralGrid', 'slice', 'total_variation_loss', 'tensor_formula', 'tv_formula', 'identity_grids']

LUMA = (0.299, 0.587, 0.114)


def identity_grids(num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8, device=None, dtype=torch.float32) -> torch.Tensor:
    """(num, 12, grid_W, grid_Y, grid_X): the identity transform at every vertex (channels 0, 5, 10 one, the rest zero)."""
    g = torch.zeros(num, 12, grid_W, grid_Y, grid_X, device=device, dtype=dtype)
    g[:, (0, 5, 10)] = 1
    return g


def _axis(t: torch.Tensor, n: int):
    """cell index (int64) and fraction of the coordinates t along an axis of n vertices."""
    if n == 1:
        return torch.zeros_like(t, dtype=torch.int64), torch.zeros_like(t)
    c = t.clamp(0, 1) * (n - 1)
    i = c.detach().floor().clamp(0, n - 2).to(torch.int64)
    return i, c - i.to(c.dtype)


def tensor_formula(grids: torch.Tensor, rgb: torch.Tensor, idx, xy: torch.Tensor | None = None, return_affine: bool = False):
    """The definition as explicit gathers (any device, any floating dtype; not built on grid_sample, so the g == 1 rule is the same everywhere).
    Image form: rgb (3, H, W) or (H, W, 3), idx one grid (int or 0-d / 1-element integer tensor).  Ray-list form: rgb (n, 3), xy (n, 2) holding (u, v) in
    [0, 1], idx (n,) integer tensor or one int.  Returns the corrected colours in rgb's layout (and the sliced matrices (..., 12) with return_affine)."""
    n_grids, _, L, Gh, Gw = grids.shape
    if xy is None:
        if rgb.dim() != 3 or (rgb.shape[0] != 3 and rgb.shape[2] != 3):
            raise RuntimeError(f'bilateral_grid: rgb must be (3, H, W) or (H, W, 3), got {tuple(rgb.shape)}')
        chw = rgb.shape[0] == 3
        p = rgb.permute(1, 2, 0) if chw else rgb                                          # (H, W, 3)
        H, W = p.shape[:2]
        u = ((torch.arange(W, device=rgb.device, dtype=rgb.dtype) + 0.5) / W)[None, :].expand(H, W)
        v = ((torch.arange(H, device=rgb.device, dtype=rgb.dtype) + 0.5) / H)[:, None].expand(H, W)
        if isinstance(idx, torch.Tensor):
            n = idx.to(rgb.device).reshape(-1)[:1].to(torch.int64).clamp(0, n_grids - 1).expand(H, W)
        else:
            n = int(idx)                                                                  # a plain integer stays on the host: nothing is copied, capturable
            if not 0 <= n < n_grids:
                raise RuntimeError(f'bilateral_grid: grid index {n} outside [0, {n_grids})')
    else:
        chw = False
        p = rgb
        u, v = xy[..., 0], xy[..., 1]
        n = idx.to(rgb.device).to(torch.int64).expand(p.shape[:-1]) if isinstance(idx, torch.Tensor) else int(idx)
    g = LUMA[0] * p[..., 0] + LUMA[1] * p[..., 1] + LUMA[2] * p[..., 2]
    (ix, fx), (iy, fy), (iz, fz) = _axis(u, Gw), _axis(v, Gh), _axis(g, L)
    G = grids.permute(0, 2, 3, 4, 1)                                                       # (N, L, Gh, Gw, 12)
    A = 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            for dz, wz in ((0, 1 - fz), (1, fz)):
                if (dz and L == 1) or (dy and Gh == 1) or (dx and Gw == 1):
                    continue
                A = A + (wz * (wy * wx))[..., None] * G[n, iz + dz, iy + dy, ix + dx]
    M = A.reshape(*A.shape[:-1], 3, 4)
    out = (M[..., :3] * p[..., None, :]).sum(-1) + M[..., 3]
    if chw:
        out = out.permute(2, 0, 1)
    return (out, A) if return_affine else out


def tv_formula(grids: torch.Tensor) -> torch.Tensor:
    """TV(G) = (1/N) sum_axis sum (G[i+1] - G[i])^2 / count_axis as tensor operations; an axis of extent 1 contributes zero."""
    total = grids.new_zeros(())
    for dim in (2, 3, 4):
        n = grids.shape[dim]
        if n > 1:
            total = total + (grids.narrow(dim, 1, n - 1) - grids.narrow(dim, 0, n - 1)).pow(2).mean()
    return total


def _idx_args(idx, device):
    """(host integer, device int32 tensor or None) of a grid index."""
    if isinstance(idx, torch.Tensor):
        if idx.numel() != 1:
            raise RuntimeError('bilateral_grid: the image form takes ONE grid index')
        if idx.is_cuda:
            if idx.dtype != torch.int32:
                raise RuntimeError('bilateral_grid: a device grid index must be int32')
            return 0, idx.reshape(1)
        return int(idx), None
    return int(idx), None


class _Slice(torch.autograd.Function):
    """out = A(p) p + b(p) as ONE node: one launch forward, two backward (nrc_bilagrid_slice_*)."""

    @staticmethod
    def forward(ctx, grids, rgb, idx, return_affine):
        lib = _lib.load()
        n_grids, _, L, Gh, Gw = grids.shape
        chw = rgb.shape[0] == 3
        H, W = (rgb.shape[1], rgb.shape[2]) if chw else (rgb.shape[0], rgb.shape[1])
        ps, cs = (1, H * W) if chw else (3, 1)
        idx_host, idx_dev = _idx_args(idx, rgb.device)
        if idx_dev is None and not 0 <= idx_host < n_grids:
            raise RuntimeError(f'bilateral_grid: grid index {idx_host} outside [0, {n_grids})')
        out = torch.empty_like(rgb)
        affine = torch.empty(H, W, 12, dtype=torch.float32, device=rgb.device) if return_affine else None
        _lib.check(lib.nrc_bilagrid_slice_forward(_lib.ptr(grids), n_grids, L, Gh, Gw, _lib.ptr(rgb), H, W, ps, cs, idx_host, _lib.ptr(idx_dev), _lib.ptr(out),
                                                  _lib.ptr(affine), _lib.stream_of(rgb)), 'bilagrid_slice_forward')
        ctx.save_for_backward(grids.detach(), rgb.detach(), idx_dev)
        ctx.args = (n_grids, L, Gh, Gw, H, W, ps, cs, idx_host)
        if return_affine:
            ctx.mark_non_differentiable(affine)
            return out, affine
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, *unused):
        grids, rgb, idx_dev = ctx.saved_tensors
        n_grids, L, Gh, Gw, H, W, ps, cs, idx_host = ctx.args
        lib = _lib.load()
        want_g, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_g or want_p):
            return None, None, None, None
        d_out = d_out.to(torch.float32).contiguous()
        d_rgb = torch.empty_like(rgb) if want_p else None
        d_grids = torch.empty_like(grids) if want_g else None
        ws = torch.empty(int(lib.nrc_bilagrid_ws_floats(n_grids, L, Gh, Gw, H, W)), dtype=torch.float32, device=rgb.device) if want_g else None
        _lib.check(lib.nrc_bilagrid_slice_backward(_lib.ptr(grids), n_grids, L, Gh, Gw, _lib.ptr(rgb), _lib.ptr(d_out), H, W, ps, cs, idx_host, _lib.ptr(idx_dev),
                                                   _lib.ptr(ws), _lib.ptr(d_rgb), _lib.ptr(d_grids), _lib.stream_of(rgb)), 'bilagrid_slice_backward')
        return d_grids, d_rgb, None, None


class _TotalVariation(torch.autograd.Function):
    """TV(G) as ONE node: two launches forward (double sums in a fixed order), one stencil backward; the upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, grids):
        lib = _lib.load()
        n_grids, _, L, Gh, Gw = grids.shape
        ws = torch.empty(int(lib.nrc_bilagrid_ws_floats(n_grids, L, Gh, Gw, 0, 0)), dtype=torch.float32, device=grids.device)
        tv = torch.empty(1, dtype=torch.float32, device=grids.device)
        _lib.check(lib.nrc_bilagrid_tv_forward(_lib.ptr(grids), n_grids, L, Gh, Gw, _lib.ptr(ws), _lib.ptr(tv), _lib.stream_of(grids)), 'bilagrid_tv_forward')
        ctx.save_for_backward(grids.detach())
        return tv[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_tv):
        grids, = ctx.saved_tensors
        n_grids, _, L, Gh, Gw = grids.shape
        g = grad_tv.to(torch.float32).reshape(1).contiguous()
        d_grids = torch.empty_like(grids)
        _lib.check(_lib.load().nrc_bilagrid_tv_backward(_lib.ptr(grids), n_grids, L, Gh, Gw, _lib.ptr(g), _lib.ptr(d_grids), _lib.stream_of(grids)),
                   'bilagrid_tv_backward')
        return d_grids


def _check_grids(grids):
    if grids.dim() != 5 or grids.shape[1] != 12 or min(grids.shape) < 1:
        raise RuntimeError(f'bilateral_grid: grids must be (N, 12, L, Gh, Gw) with every extent >= 1, got {tuple(grids.shape)}')


def slice(grids: torch.Tensor, rgb: torch.Tensor, idx, xy: torch.Tensor | None = None, return_affine: bool = False):
    """Colour-correct `rgb` with grid `idx` of `grids` (N, 12, L, Gh, Gw).  Image form: rgb (3, H, W) or (H, W, 3) -- a (3, W, 3) tensor is read as (3, H, W) --
    and ONE index: an int, or an int32 tensor on the device (read by the kernels, so a captured graph can change it).  Ray-list form: rgb (n, 3),
    xy (n, 2) = (u, v) in [0, 1], idx (n,) or an int; it takes the tensor formula.  Gradients flow to grids and rgb, not to xy."""
    _check_grids(grids)
    if xy is not None:
        return tensor_formula(grids, rgb, idx, xy, return_affine)
    if rgb.dim() != 3 or (rgb.shape[0] != 3 and rgb.shape[2] != 3):
        raise RuntimeError(f'bilateral_grid: rgb must be (3, H, W) or (H, W, 3), got {tuple(rgb.shape)}')
    if not (grids.is_cuda and rgb.is_cuda and grids.dtype == rgb.dtype == torch.float32) or rgb.numel() == 0:
        return tensor_formula(grids, rgb, idx, None, return_affine)
    return _Slice.apply(grids.contiguous(), rgb.contiguous(), idx, bool(return_affine))


def total_variation_loss(grids: torch.Tensor) -> torch.Tensor:
    """TV(G) = (1/N) sum_{axis in z,y,x} sum (G[.., i+1, ..] - G[.., i, ..])^2 / count_axis: the mean squared forward difference per axis, summed."""
    _check_grids(grids)
    if not (grids.is_cuda and grids.dtype == torch.float32):
        return tv_formula(grids)
    return _TotalVariation.apply(grids.contiguous())


class BilateralGrid(torch.nn.Module):
    """`num` grids of grid_W x grid_Y x grid_X vertices (luminance, y, x), one per training image, initialised to the identity.
    forward(rgb, idx) corrects a rendered image with grid idx; tv_loss() is the regulariser (gsplat weights it with 10)."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8) -> None:
        super().__init__()
        self.grids = torch.nn.Parameter(identity_grids(num, grid_X, grid_Y, grid_W))

    def forward(self, rgb: torch.Tensor, idx, return_affine: bool = False):
        return slice(self.grids, rgb, idx, None, return_affine)

    def tv_loss(self) -> torch.Tensor:
        return total_variation_loss(self.grids)
