"""nerficg_amd.gaussian_splatting -- host-side mirror of the reference's GaussianSplatting call sites into the rasterizer
(src/Methods/GaussianSplatting/Renderer.py:51-86,158-184), its activation accessors (Model.py:45-87) and the PyTorch
helpers that double as in-tree oracles for two rasterizer sub-steps (utils.py:10-59, Cameras/utils.py:180-208,
Cameras/Perspective.py:96-119).  Pure torch + nerficg_amd.diff_gaussian_rasterization; the helpers run on CPU too
(they are pinned against the reference's golden vectors in tests/test_host_golden.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

__all__ = ['PerspectiveCamera', 'get_projection_matrix', 'invert_3d_affine', 'make_raster_settings', 'quaternion_to_rotation_matrix',
           'build_covariances', 'extract_upper_triangular_matrix', 'sh_basis', 'convert_sh_features', 'rgb_to_sh0', 'sh0_to_rgb', 'Gaussians',
           'render_image_training', 'render_image_inference', 'training_loss', 'rest_step_schedule', 'RestStep', 'band_parallel_training_step', 'mcmc_noise',
           'mcmc_regulariser_grads']


@dataclass
class PerspectiveCamera:
    """Fields of src/Cameras/Perspective.py:16-37 + SharedCameraSettings that the 3DGS path reads."""
    width: int
    height: int
    focal_x: float
    focal_y: float
    center_x: float | None = None
    center_y: float | None = None
    near_plane: float = 0.01
    far_plane: float = 100.0
    background_color: torch.Tensor | None = None

    def __post_init__(self) -> None:
        if self.center_x is None:
            self.center_x = self.width / 2
        if self.center_y is None:
            self.center_y = self.height / 2
        if self.background_color is None:
            self.background_color = torch.zeros(3)


def get_projection_matrix(cam: PerspectiveCamera, invert_z: bool = False, device=None) -> torch.Tensor:
    """Cameras/Perspective.py:96-119 (OpenGL-style clip matrix, x/y/z in [-1,1] after the perspective division)."""
    half_width, half_height = cam.width * 0.5, cam.height * 0.5
    offset_x, offset_y = cam.center_x - half_width, cam.center_y - half_height
    z_sign = -1.0 if invert_z else 1.0
    f, n = cam.far_plane, cam.near_plane
    return torch.tensor([
        [cam.focal_x / half_width, 0.0, z_sign * offset_x / half_width, 0.0],
        [0.0, cam.focal_y / half_height, z_sign * offset_y / half_height, 0.0],
        [0.0, 0.0, z_sign * (f + n) / (f - n), -2.0 * f * n / (f - n)],
        [0.0, 0.0, z_sign, 0.0]], dtype=torch.float32, device=device)


def invert_3d_affine(transform: np.ndarray) -> np.ndarray:
    """Cameras/utils.py:211-222 for rigid transforms."""
    inv = np.eye(4, dtype=transform.dtype)
    inv[:3, :3] = transform[:3, :3].T
    inv[:3, 3] = transform[:3, :3].T @ -transform[:3, 3]
    return inv


_PROJECTIONS: dict = {}


def _projection_transposed(cam: PerspectiveCamera, device) -> torch.Tensor:
    """P.T of get_projection_matrix on `device`, built once per camera geometry (a host -> device copy per frame otherwise)."""
    key = (cam.width, cam.height, cam.focal_x, cam.focal_y, cam.center_x, cam.center_y, cam.near_plane, cam.far_plane, str(device))
    hit = _PROJECTIONS.get(key)
    if hit is None:
        if len(_PROJECTIONS) >= 64:
            _PROJECTIONS.pop(next(iter(_PROJECTIONS)))
        hit = _PROJECTIONS[key] = get_projection_matrix(cam, device=device).T.contiguous()
    return hit


class _CameraBlock(torch.autograd.Function):
    """The rasterizer's camera block (view | view @ P^T | position | background, float[38]) of a device pose that requires grad: forward nrc_gs_camera_block,
    backward its transpose nrc_gs_camera_block_backward (one launch of one wave each).  The background receives no gradient."""

    @staticmethod
    def forward(ctx, pose, proj_t, bg):
        from . import _lib
        block = torch.empty(38, dtype=torch.float32, device=pose.device)
        _lib.check(_lib.load().nrc_gs_camera_block(_lib.ptr(pose), _lib.ptr(proj_t), _lib.ptr(bg), _lib.ptr(block), _lib.stream_of(block)), 'gs_camera_block')
        ctx.save_for_backward(pose, proj_t)
        return block

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_block):
        from . import _lib
        pose, proj_t = ctx.saved_tensors
        d_block = d_block.to(torch.float32).contiguous()
        d_pose = torch.zeros_like(pose)      # ((4, 4): the last row is not read by the forward)
        _lib.check(_lib.load().nrc_gs_camera_block_backward(_lib.ptr(pose), _lib.ptr(proj_t), _lib.ptr(d_block), _lib.ptr(d_pose), _lib.stream_of(d_pose)),
                   'gs_camera_block_backward')
        return d_pose, None, None


def make_raster_settings(cam: PerspectiveCamera, c2w, sh_degree: int, scale_modifier: float = 1.0, device='cuda'):
    """GaussianSplatting/Renderer.py:60-74: viewmatrix = w2c.T, projmatrix = w2c.T @ P.T, tanfov = size / focal / 2.  `c2w`: a (4,4) / (3,4)
    array, or a device tensor -- the pose then never visits the host (w2c.T = [[R, 0], [-(R^T t)^T, 1]] is assembled by torch on the
    device), which is what a recorded training step needs: it re-reads the tensor on every replay.  A device tensor that requires grad: the
    settings' viewmatrix / projmatrix / campos carry the graph back to it (rasterize with camera_grad=True)."""
    from .diff_gaussian_rasterization import GaussianRasterizationSettings
    if torch.is_tensor(c2w) and c2w.is_cuda:
        # one launch writes the rasterizer's whole camera block (view | view @ P^T | position | background); the settings' tensors are views of it and
        # the rasterizer recognises the block (diff_gaussian_rasterization.adopt_camera_block) instead of concatenating its own
        from . import _lib
        from .diff_gaussian_rasterization import adopt_camera_block
        pose = c2w.to(device=device, dtype=torch.float32).contiguous()
        bg = cam.background_color.to(device=device, dtype=torch.float32).contiguous()
        if pose.requires_grad and torch.is_grad_enabled():
            if pose.shape[-2:] not in ((3, 4), (4, 4)) or pose.dim() != 2:
                raise RuntimeError(f'make_raster_settings: c2w (3, 4) or (4, 4) expected, got {tuple(pose.shape)}')
            block = _CameraBlock.apply(pose, _projection_transposed(cam, device), bg)
        else:
            block = torch.empty(38, dtype=torch.float32, device=pose.device)
            _lib.check(_lib.load().nrc_gs_camera_block(_lib.ptr(pose), _lib.ptr(_projection_transposed(cam, device)), _lib.ptr(bg), _lib.ptr(block), _lib.stream_of(block)),
                       'gs_camera_block')
        adopt_camera_block(block.detach())      # (the rasterizer recognises the block by its address)
        return GaussianRasterizationSettings(
            image_height=cam.height, image_width=cam.width, tanfovx=cam.width / cam.focal_x * 0.5, tanfovy=cam.height / cam.focal_y * 0.5,
            bg=block[35:38], scale_modifier=scale_modifier, viewmatrix=block[:16].view(4, 4), projmatrix=block[16:32].view(4, 4), sh_degree=sh_degree,
            campos=block[32:35], prefiltered=False, debug=False)
    elif torch.is_tensor(c2w):
        pose = c2w.to(device=device, dtype=torch.float32)
        rot, pos = pose[:3, :3], pose[:3, 3]
        last_row = torch.cat([-(rot.T @ pos), pose.new_ones(1)])
        view = torch.cat([torch.cat([rot, pose.new_zeros(3, 1)], dim=1), last_row[None]], dim=0)
        campos = pos.contiguous()
    else:
        c2w = np.asarray(c2w, dtype=np.float64)
        view = torch.as_tensor(invert_3d_affine(c2w), dtype=torch.float32, device=device).T
        campos = torch.as_tensor(c2w[:3, 3], dtype=torch.float32, device=device)
    return GaussianRasterizationSettings(
        image_height=cam.height, image_width=cam.width, tanfovx=cam.width / cam.focal_x * 0.5, tanfovy=cam.height / cam.focal_y * 0.5,
        bg=cam.background_color.to(device), scale_modifier=scale_modifier, viewmatrix=view,
        projmatrix=view @ _projection_transposed(cam, device), sh_degree=sh_degree, campos=campos, prefiltered=False, debug=False)


def quaternion_to_rotation_matrix(quaternions: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """(..., 4) quaternions, real part first -> (..., 3, 3) rotation matrices (same convention and values as Cameras/utils.py:180-208):
    the nine entries of R = I + 2 (w [v]x + [v]x [v]x), v = vector part, stacked row by row."""
    q = torch.nn.functional.normalize(quaternions, dim=-1) if normalize else quaternions
    w, x, y, z = q.unbind(-1)
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(rows, dim=-1).reshape(*q.shape[:-1], 3, 3)


_UPPER_ROWS, _UPPER_COLS = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)


def build_covariances(scales: torch.Tensor, rotations: torch.Tensor) -> torch.Tensor:
    """Sigma = (R diag(s)) (R diag(s))^T for unit quaternions `rotations` (the rasterizer's cov3D step; GaussianSplatting/utils.py:10-18).
    Scaling the columns of R replaces the product with a diagonal matrix."""
    stretched = quaternion_to_rotation_matrix(rotations, normalize=False) * scales[..., None, :]
    return stretched @ stretched.mT


def extract_upper_triangular_matrix(matrix: torch.Tensor) -> torch.Tensor:
    """Row-major upper triangle of (..., n, n) matrices; (..., 6) for the 3x3 covariances the rasterizer takes as cov3D_precomp."""
    n = matrix.shape[-1]
    if n == 3:
        return matrix[..., _UPPER_ROWS, _UPPER_COLS]
    rows, cols = zip(*[(r, c) for r in range(n) for c in range(r, n)])
    return matrix[..., rows, cols]


# real spherical-harmonics basis up to degree 3 in the sign / order convention of 3DGS (GaussianSplatting/utils.py:27-58): constants first,
# then the polynomial each one multiplies
_SH_C = (0.28209479177387814,
         -0.48860251190291987, 0.48860251190291987, -0.48860251190291987,
         1.0925484305920792, -1.0925484305920792, 0.94617469575755997, -1.0925484305920792, 0.54627421529603959,
         0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 0.45704579946446572, 1.4453057213202769, 0.59004358992664352)


def sh_basis(directions: torch.Tensor, degree: int) -> torch.Tensor:
    """(..., 3) unit directions -> (..., (degree+1)^2) basis values."""
    x, y, z = directions.unbind(-1)
    one = torch.ones_like(x)
    poly = [one]
    if degree >= 1:
        poly += [y, z, x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        poly += [x * y, y * z, zz - 0.31539156525251999 / 0.94617469575755997, x * z, xx - yy]
    if degree >= 3:
        poly += [y * (yy - 3.0 * xx), x * y * z, y * (1.0 - 5.0 * zz), z * (5.0 * zz - 3.0), x * (1.0 - 5.0 * zz), z * (xx - yy), x * (3.0 * yy - xx)]
    basis = torch.stack(poly, dim=-1)
    return basis * torch.tensor(_SH_C[:len(poly)], dtype=basis.dtype, device=basis.device)


def convert_sh_features(sh_features: torch.Tensor, view_directions: torch.Tensor, degree: int) -> torch.Tensor:
    """SH coefficients (..., 3, 16) seen from view_directions (..., 1|3 broadcastable, 3) -> RGB = max(0, 0.5 + sum_k Y_k c_k): the rasterizer's
    colour step in torch (the reference's utils.py:21-59 is pinned against this in tests/test_host_golden.py)."""
    n = (degree + 1) ** 2
    basis = sh_basis(view_directions[..., 0, :] if view_directions.dim() == sh_features.dim() else view_directions, degree)
    return ((sh_features[..., :n] * basis[..., None, :]).sum(-1) + 0.5).clamp_min(0.0)


def rgb_to_sh0(rgb):
    return (rgb - 0.5) / _SH_C[0]


def sh0_to_rgb(sh):
    return sh * _SH_C[0] + 0.5


def _mcmc_draw(probabilities: torch.Tensor, n: int) -> torch.Tensor:
    """n indices drawn with replacement (torch.multinomial, as the published 3DGS-MCMC does)."""
    if probabilities.numel() > 2 ** 24:
        raise RuntimeError(f'3DGS-MCMC sampling: torch.multinomial takes at most 2^24 categories, {probabilities.numel()} rows given; '
                           'draw the rows yourself and pass them as sampled=')
    return torch.multinomial(probabilities, n, replacement=True)


def _mcmc_relocation(opacity_logits: torch.Tensor, log_scales: torch.Tensor, counts: torch.Tensor, moments: list[torch.Tensor],
                     opacity_out: torch.Tensor | None = None, scales_out: torch.Tensor | None = None) -> None:
    """nrc_gs_mcmc_relocation in place on (P, 1) logits and (P, 3) log-scales for the rows with counts > 0; `moments` (at most 12 tensors of P rows) lose
    those rows.  opacity_out (P) / scales_out (P, 3): optional, receive the new activated values of those rows."""
    import ctypes
    from . import _lib
    _lib.check_input(opacity_logits, 'opacity logits', torch.float32)
    _lib.check_input(log_scales, 'log scales', torch.float32)
    _lib.check_input(counts, 'counts', torch.int32)
    P = opacity_logits.shape[0]
    if log_scales.shape[0] != P or counts.numel() != P:
        raise RuntimeError('mcmc relocation: logits, log-scales and counts must have the same number of rows')
    for m in moments:
        _lib.check_input(m, 'Adam moment', torch.float32)
        if m.shape[0] != P:
            raise RuntimeError('mcmc relocation: a moment tensor with another number of rows')
    for t in (opacity_out, scales_out):
        if t is not None:
            _lib.check_input(t, 'relocation output', torch.float32)
    n = len(moments)
    a_ptr = (ctypes.c_void_p * max(n, 1))(*[m.data_ptr() for m in moments])
    a_row = (ctypes.c_int32 * max(n, 1))(*[max(1, int(np.prod(m.shape[1:]))) for m in moments])
    _lib.check(_lib.load().nrc_gs_mcmc_relocation(_lib.ptr(opacity_logits), _lib.ptr(log_scales), _lib.ptr(counts), P, ctypes.cast(a_ptr, ctypes.c_void_p),
                                                  ctypes.cast(a_row, ctypes.c_void_p), n, _lib.ptr(opacity_out), _lib.ptr(scales_out),
                                                  _lib.stream_of(opacity_logits)), 'gs_mcmc_relocation')


def mcmc_noise(positions: torch.Tensor, rotations: torch.Tensor, log_scales: torch.Tensor, opacity_logits: torch.Tensor, lr: float, noise_lr: float = 5e5,
               seed: int = 0, iteration: int = 0, z: torch.Tensor | None = None, z_out: torch.Tensor | None = None, row_offset: int = 0,
               lr_dev: torch.Tensor | None = None, device_step: torch.Tensor | None = None) -> None:
    """nrc_gs_mcmc_noise in place on `positions` (P, 3): x += R diag(s^2) R^T (z * gate * noise_lr * lr).  row_offset: the global row of local row 0 (the
    generator's counter is the global row, so a model cut into several launches, or over ranks, draws what one launch draws).  lr_dev (device f32[1]) /
    device_step (device i32[1]) replace lr / iteration."""
    from . import _lib
    for t, name in ((positions, 'positions'), (rotations, 'rotations'), (log_scales, 'log scales'), (opacity_logits, 'opacity logits'), (z, 'z'), (z_out, 'z_out'),
                    (lr_dev, 'lr_dev')):
        if t is not None:
            _lib.check_input(t, name, torch.float32)
    if device_step is not None:
        _lib.check_input(device_step, 'device_step', torch.int32)
    P = positions.shape[0]
    if rotations.shape[0] != P or log_scales.shape[0] != P or opacity_logits.shape[0] != P or any(t is not None and tuple(t.shape) != (P, 3) for t in (z, z_out)):
        raise RuntimeError('mcmc_noise: P rows expected in every tensor, (P, 3) for z and z_out')
    if iteration < 0 or row_offset < 0:
        raise RuntimeError('mcmc_noise: iteration and row_offset must not be negative')
    _lib.check(_lib.load().nrc_gs_mcmc_noise(_lib.ptr(rotations), _lib.ptr(log_scales), _lib.ptr(opacity_logits), _lib.ptr(positions), P, int(row_offset),
                                             float(noise_lr), float(lr), _lib.ptr(lr_dev), int(seed) & (2 ** 64 - 1), int(iteration), _lib.ptr(device_step),
                                             _lib.ptr(z), _lib.ptr(z_out), _lib.stream_of(positions)), 'gs_mcmc_noise')


def mcmc_regulariser_grads(opacity_logits: torch.Tensor, log_scales: torch.Tensor, grad_opacity_logits: torch.Tensor, grad_log_scales: torch.Tensor,
                           opacity_reg: float = 0.01, scale_reg: float = 0.01) -> torch.Tensor:
    """nrc_gs_mcmc_regularise: adds d(opacity_reg * mean(o)) / d logit and d(scale_reg * mean(s)) / d log_scale to the two gradient tensors in place and
    returns the device tensor [L_o, L_s]."""
    from . import _lib
    for t, name in ((opacity_logits, 'opacity logits'), (log_scales, 'log scales'), (grad_opacity_logits, 'opacity gradient'), (grad_log_scales, 'scale gradient')):
        _lib.check_input(t, name, torch.float32)
    P = opacity_logits.shape[0]
    if log_scales.shape[0] != P or grad_opacity_logits.numel() != P or grad_log_scales.numel() != 3 * P:
        raise RuntimeError('mcmc_regulariser_grads: (P, 1) logits and (P, 3) log-scales with gradients of the same shapes expected')
    lib = _lib.load()
    losses = torch.zeros(2, dtype=torch.float32, device=opacity_logits.device)
    ws = torch.empty(max(1, int(lib.nrc_gs_mcmc_regularise_ws_bytes(P)) // 8), dtype=torch.float64, device=opacity_logits.device)
    _lib.check(lib.nrc_gs_mcmc_regularise(_lib.ptr(opacity_logits), _lib.ptr(log_scales), P, float(opacity_reg), float(scale_reg), _lib.ptr(grad_opacity_logits),
                                          _lib.ptr(grad_log_scales), _lib.ptr(losses), _lib.ptr(ws), _lib.stream_of(opacity_logits)), 'gs_mcmc_regularise')
    return losses


def filter_3d(positions: torch.Tensor, views: torch.Tensor) -> torch.Tensor:
    """(P,) float32: nrc_gs_filter3d on positions (P, 3) and a (V, 20) float32 block of views on the same device -- per view the world-to-camera matrix row-major
    (p_cam = m[:3, :3] p + m[:3, 3]), fx, fy, W, H.  See Gaussians.compute_3d_filter."""
    from . import _lib
    if not positions.is_cuda or views.device != positions.device:
        raise RuntimeError('filter_3d: positions and views must be CUDA tensors on one device')
    if positions.dim() != 2 or positions.shape[1] != 3 or views.dim() != 2 or views.shape[1] != 20 or views.shape[0] < 1:
        raise RuntimeError(f'filter_3d: positions (P, 3) and views (V >= 1, 20) expected, got {tuple(positions.shape)} and {tuple(views.shape)}')
    pos = positions.detach().to(torch.float32).contiguous()
    blk = views.detach().to(torch.float32).contiguous()
    out = torch.empty(pos.shape[0], dtype=torch.float32, device=pos.device)
    ws = torch.empty(1, dtype=torch.int32, device=pos.device)
    _lib.check(_lib.load().nrc_gs_filter3d(_lib.ptr(pos), pos.shape[0], _lib.ptr(blk), blk.shape[0], _lib.ptr(out), _lib.ptr(ws), _lib.stream_of(out)), 'gs_filter3d')
    return out


class Gaussians(torch.nn.Module):
    """Parameter store + activation accessors of GaussianSplatting/Model.py:18-87 (exp scales, normalised quaternions, sigmoid
    opacities, cat[dc, rest] SH features of shape (P, 16, 3)) and the training-time bookkeeping of Model.py:94-284: optimizer setup,
    densification statistics, densify_and_prune, opacity reset, activation baking, ply export.  The bookkeeping runs on the device through
    include/nerficg_hip.h group 10 (one classification + scan, one gather over all parameters and Adam moments)."""

    def __init__(self, positions, log_scales, rotations, opacity_logits, features_dc, features_rest, sh_degree: int = 3) -> None:
        super().__init__()
        P = torch.nn.Parameter
        self._positions, self._scales, self._rotations = P(positions), P(log_scales), P(rotations)
        self._opacities, self._features_dc, self._features_rest = P(opacity_logits), P(features_dc), P(features_rest)
        self.active_sh_degree = sh_degree
        self.max_sh_degree = sh_degree
        self.optimizer = None
        self.percent_dense = 0.0
        self.training_cameras_extent = 1.0
        self.baked = False
        self._baked_covariances = None
        n, dev = positions.shape[0], positions.device
        self.densification_gradient_accum = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        self.n_observations = torch.zeros((n, 1), dtype=torch.int32, device=dev)
        self.filter_3D = None   # (P, 1) after compute_3d_filter(views); None again whenever the rows change

    @classmethod
    def from_point_cloud(cls, positions: torch.Tensor, colors: torch.Tensor | None = None, sh_degree: int = 3) -> 'Gaussians':
        """initialize_from_point_cloud (Model.py:94-119): isotropic scales from the RMS distance to the 3 nearest neighbours
        (Optim/knn_utils.py:29-40 through the HIP kNN), identity rotations, opacity 0.1, DC colour from rgb."""
        from .simple_knn import distCUDA2
        xyz = positions.to(torch.float32).contiguous()
        n, dev = xyz.shape[0], xyz.device
        n_coeff = (sh_degree + 1) ** 2
        base_colour = torch.full((n, 3), 0.5, device=dev) if colors is None else colors.to(dev, torch.float32)
        dc = rgb_to_sh0(base_colour).reshape(n, 1, 3).contiguous()                       # (P, 1, 3): coefficient-major like the rasterizer reads it
        rest = torch.zeros(n, n_coeff - 1, 3, device=dev)
        spacing = distCUDA2(xyz).clamp_min(1e-7).sqrt()                                  # RMS distance to the three nearest neighbours
        log_scales = spacing.log().reshape(n, 1).expand(n, 3).contiguous()
        identity = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).expand(n, 4).contiguous()
        opacity_logits = torch.full((n, 1), float(np.log(0.1 / 0.9)), device=dev)        # logit(0.1)
        out = cls(xyz, log_scales, identity, opacity_logits, dc, rest, sh_degree)
        out.active_sh_degree = 0
        return out

    @property
    def get_positions(self): return self._positions
    @property
    def get_scales(self): return self._scales if self.baked else torch.exp(self._scales)
    @property
    def get_rotations(self): return self._rotations if self.baked else torch.nn.functional.normalize(self._rotations)
    @property
    def get_opacities(self): return self._opacities if self.baked else torch.sigmoid(self._opacities)
    @property
    def get_features_dc(self): return self._features_dc
    @property
    def get_features_rest(self): return self._features_rest
    @property
    def get_features(self): return torch.cat((self._features_dc, self._features_rest), dim=1)
    @property
    def get_baked_covariances(self): return self._baked_covariances

    # ---------------------------------------------------------------- the 3-D smoothing filter of Mip-Splatting
    def _checked_filter_3d(self) -> torch.Tensor:
        f = self.filter_3D
        if f is None:
            raise RuntimeError('the 3-D filter is not set: call compute_3d_filter(views) first (and again after every change of the number of Gaussians)')
        if f.shape[0] != self._positions.shape[0]:
            raise RuntimeError(f'filter_3D holds {f.shape[0]} rows, the model {self._positions.shape[0]} Gaussians: call compute_3d_filter(views) again')
        return f

    @property
    def get_scales_with_3d_filter(self):
        """sqrt(s^2 + f^2): the scales of the Gaussian convolved with the isotropic low-pass of width filter_3D (Mip-Splatting).  Plain differentiable torch."""
        s = self.get_scales
        return torch.sqrt(torch.square(s) + torch.square(self._checked_filter_3d()))

    @property
    def get_opacities_with_3d_filter(self):
        """o sqrt(prod s^2 / prod (s^2 + f^2)): the opacity that keeps the Gaussian's integral under that convolution (Mip-Splatting).  Plain differentiable torch."""
        s2 = torch.square(self.get_scales)
        f2 = torch.square(self._checked_filter_3d())
        return self.get_opacities * torch.sqrt(torch.prod(s2, dim=1) / torch.prod(s2 + f2, dim=1))[..., None]

    @torch.no_grad()
    def compute_3d_filter(self, views) -> torch.Tensor:
        """Fills self.filter_3D, (P, 1): sqrt(0.2) times the smallest z / fx over the views that see the Gaussian -- the largest sampling rate any training view
        has of it, as a Gaussian low-pass in world units (Mip-Splatting's compute_3D_filter; one kernel, nrc_gs_filter3d).  `views`: an iterable of
        (PerspectiveCamera, c2w).  A view sees a Gaussian iff its view-space z > 0.2 and its pixel lies in the frame widened by 15 % on every side; a Gaussian
        that no view sees gets the largest filter among the seen ones.  The published code divides the smallest z by the largest focal length of all views;
        the per-view ratio z / fx used here equals it for equal focal lengths.  Any change of the number of Gaussians (prune_points, densify_and_prune,
        relocate, add_new) sets filter_3D back to None: call this again, as Mip-Splatting does after every densification."""
        pos = self._positions.detach().to(torch.float32).contiguous()
        dev = pos.device
        rows = []
        for cam, c2w in views:
            pose = torch.as_tensor(np.asarray(c2w.detach().cpu()) if torch.is_tensor(c2w) else np.asarray(c2w), dtype=torch.float64)
            m = torch.eye(4, dtype=torch.float64)
            m[:3, :4] = pose[:3, :4]
            w2c = torch.linalg.inv(m)
            rows.append(torch.cat([w2c.reshape(-1), torch.tensor([cam.focal_x, cam.focal_y, cam.width, cam.height], dtype=torch.float64)]))
        if not rows:
            raise RuntimeError('compute_3d_filter: at least one view is needed')
        block = torch.stack(rows).to(device=dev, dtype=torch.float32).contiguous()
        self.filter_3D = filter_3d(pos, block)[:, None]
        return self.filter_3D

    def get_covariances(self, scale_modifier: float) -> torch.Tensor:
        """Model.py:84-86"""
        return extract_upper_triangular_matrix(build_covariances(self.get_scales * scale_modifier, self.get_rotations))

    def increase_used_sh_degree(self) -> None:
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---------------------------------------------------------------- optimizer (Model.py:121-150)
    _GROUP_OF = {'positions': '_positions', 'f_dc': '_features_dc', 'f_rest': '_features_rest', 'opacities': '_opacities', 'scales': '_scales',
                 'rotations': '_rotations'}

    def training_setup(self, LEARNING_RATE_POSITION_INIT: float = 0.00016, LEARNING_RATE_POSITION_FINAL: float = 0.0000016,
                       LEARNING_RATE_POSITION_MAX_STEPS: int = 30000, LEARNING_RATE_FEATURE: float = 0.0025, LEARNING_RATE_OPACITY: float = 0.05,
                       LEARNING_RATE_SCALING: float = 0.005, LEARNING_RATE_ROTATION: float = 0.001, PERCENT_DENSE: float = 0.01,
                       training_cameras_extent: float | None = None, optimizer_class=None, capturable: bool = False, sparse_adam: bool = False,
                       bias_correction: bool = True) -> None:
        """Six single-tensor groups in the reference's order and names; FusedAdam(lr=0, eps=1e-15, adam_w_mode=False) over the HIP step.
        capturable: step counters and learning rates on the device, for steps recorded in a HIP graph (nerficg_amd.graphs).
        sparse_adam (default False: the dense step, nothing changes): `optimizer_step(radii)` updates only the Gaussians the frame saw (radii > 0); the others
        keep their parameters and both moments untouched instead of decaying them -- Taming-3DGS, 3DGS `--optimizer_type sparse_adam`, gsplat `SelectiveAdam`.
        Another optimisation trajectory than the dense step, hence opt-in; it needs the library's FusedAdam (RuntimeError with `optimizer_class`) and excludes
        the in-backward f_rest step, which is dense over all rows (render_image_training).
        bias_correction (passed to FusedAdam; default True, as before): the published sparse kernels apply no bias correction; False selects that formula in
        this project's own operation order (csrc/adam_math.h with bc = 1).  The result equals the published kernels' within rounding, not bit for bit: they
        round (-lr m) / (sqrt(v) + eps), this step rounds lr (m / (sqrt(v) + eps)).  Ignored with `optimizer_class`."""
        from .lr_utils import LRDecayPolicy
        if training_cameras_extent is not None:
            self.training_cameras_extent = training_cameras_extent
        self.percent_dense = PERCENT_DENSE
        ext = self.training_cameras_extent
        rates = {'positions': LEARNING_RATE_POSITION_INIT * ext, 'f_dc': LEARNING_RATE_FEATURE, 'f_rest': LEARNING_RATE_FEATURE / 20.0,
                 'opacities': LEARNING_RATE_OPACITY, 'scales': LEARNING_RATE_SCALING, 'rotations': LEARNING_RATE_ROTATION}
        # one single-tensor group per attribute, in the order and under the names the reference's optimizer-state surgery looks up (Model.py:121-130)
        param_groups = [{'name': name, 'lr': rates[name], 'params': [getattr(self, attr)]} for name, attr in self._GROUP_OF.items()]
        if sparse_adam and optimizer_class is not None:
            raise RuntimeError('training_setup: sparse_adam=True needs the library\'s FusedAdam (its step(visibility=...)); leave optimizer_class unset')
        self.sparse_adam = bool(sparse_adam)
        if optimizer_class is None:
            from .apex_optimizers import FusedAdam
            self.optimizer = FusedAdam(param_groups, lr=0.0, eps=1e-15, adam_w_mode=False, capturable=capturable, bias_correction=bias_correction)
        else:
            self.optimizer = optimizer_class(param_groups, lr=0.0, eps=1e-15)
        self.position_lr_scheduler = LRDecayPolicy(lr_init=LEARNING_RATE_POSITION_INIT * ext, lr_final=LEARNING_RATE_POSITION_FINAL * ext,
                                                   max_steps=LEARNING_RATE_POSITION_MAX_STEPS)

    def optimizer_step(self, radii: torch.Tensor | None = None) -> None:
        """The optimizer's step of one iteration.  With training_setup(sparse_adam=True): `radii` is the frame's out['radii'] (or any (P,) bool / uint8 / int32
        mask; a band or data-parallel caller passes the mask that covers every contribution to the summed gradient, e.g. the union of the band_masks) and only
        its visible rows are stepped; leaving it out raises -- a silent dense step would be a different optimizer.  Otherwise the dense step."""
        if getattr(self, 'sparse_adam', False):
            if radii is None:
                raise RuntimeError('optimizer_step: this model was set up with sparse_adam=True -- pass the frame\'s radii (out[\'radii\']); a dense step here would '
                                   'be a different optimizer')
            self.optimizer.step(visibility=radii)
        else:
            self.optimizer.step()

    def update_learning_rate(self, iteration: int) -> None:
        rate = self.position_lr_scheduler(iteration)
        for group in self.optimizer.param_groups:
            if group['name'] == 'positions':
                group['lr'] = rate
        # the reference's trainer calls this first thing in iteration `iteration - 1` (Trainer.py:84): with a schedule installed the in-backward f_rest step is
        # switched per iteration, off where densify_and_prune will run between the backward pass and optimizer.step() (rest_step_schedule below)
        schedule = getattr(self, 'fuse_rest_schedule', None)
        if schedule is not None:
            self.fuse_rest_step = bool(schedule(iteration - 1))

    def _adopt(self, tensors: dict[str, torch.Tensor]) -> None:
        for name, attr in self._GROUP_OF.items():
            setattr(self, attr, tensors[name])
        self.filter_3D = None   # the rows changed: the caller computes the 3-D filter again

    # ---------------------------------------------------------------- densification (Model.py:152-246)
    def reset_opacities(self) -> None:
        from .adam_utils import replace_param_group_data
        capped = torch.special.logit(self.get_opacities.clamp(max=0.01))  # Model.py:152-155
        replace_param_group_data(self.optimizer, capped, 'opacities')

    def prune_points(self, prune_mask: torch.Tensor) -> None:
        from .adam_utils import compact_mask, gather_param_groups, gather_rows
        idx = compact_mask(~prune_mask)
        self._adopt(gather_param_groups(self.optimizer, idx, idx.numel(), None, None, 'prune_param_groups'))
        self.densification_gradient_accum, n_obs = gather_rows([self.densification_gradient_accum, self.n_observations.view(torch.float32)],
                                                               idx, idx.numel())
        self.n_observations = n_obs.view(torch.int32)

    @torch.no_grad()
    def prune_by_contribution(self, stats: dict, min_weight_max: float | None = None, min_hits: int | None = None,
                              keep_fraction: float | None = None) -> dict[str, int]:
        """Removes the Gaussians that the statistics of accumulate_contributions (or GaussianRasterizer.contributions) score low, through prune_points, so the
        optimizer state follows as it does for densification.  A Gaussian goes when ANY given criterion says so:
            min_weight_max   its largest blending weight over the views is below the threshold (RadSplat prunes at 0.01 .. 0.25);
            min_hits         fewer pixels than this blended it (min_hits=1: nothing ever saw it);
            keep_fraction    it is outside the top ceil(keep_fraction P) by 'weight_sum' (the importance sum; with an error map as pixel weights, an
                             error-weighted score): the k-th value is taken with torch.kthvalue on the device and ties at the threshold are kept.
        Returns {'pruned': n, 'kept': n}.  ValueError: no criterion, a keep_fraction outside [0, 1], a statistic a criterion needs is missing, or `stats`
        belongs to another number of Gaussians."""
        if min_weight_max is None and min_hits is None and keep_fraction is None:
            raise ValueError('prune_by_contribution: give at least one of min_weight_max, min_hits and keep_fraction')
        P, dev = self._positions.shape[0], self._positions.device
        needed = [k for k, v in (('weight_max', min_weight_max), ('hits', min_hits), ('weight_sum', keep_fraction)) if v is not None]
        for k in needed:
            t = stats.get(k)
            if not torch.is_tensor(t):
                raise ValueError(f'prune_by_contribution: stats has no {k!r}, which the given criterion needs')
            if tuple(t.shape) != (P,):
                raise ValueError(f'prune_by_contribution: stats[{k!r}] has shape {tuple(t.shape)}, the model holds {P} Gaussians -- statistics of another model state')
        prune = torch.zeros(P, dtype=torch.bool, device=dev)
        if min_weight_max is not None:
            prune |= stats['weight_max'].to(dev) < float(min_weight_max)
        if min_hits is not None:
            prune |= stats['hits'].to(dev) < int(min_hits)
        if keep_fraction is not None:
            if not 0.0 <= float(keep_fraction) <= 1.0:
                raise ValueError(f'prune_by_contribution: keep_fraction = {keep_fraction}, a fraction in [0, 1] is needed')
            n_keep = min(P, int(np.ceil(float(keep_fraction) * P)))
            if n_keep == 0:
                prune |= True
            elif n_keep < P:
                score = stats['weight_sum'].to(dev)
                threshold = torch.kthvalue(score, P - n_keep + 1).values      # the n_keep-th largest; stays on the device
                prune |= score < threshold
        n_pruned = int(prune.sum())
        if n_pruned > 0:
            self.prune_points(prune)
        return {'pruned': n_pruned, 'kept': P - n_pruned}

    @torch.no_grad()
    def add_densification_stats(self, viewspace_point_tensor: torch.Tensor, visibility: torch.Tensor, use_absgrad: bool = False) -> None:
        """Model.py:243-246.  `visibility`: the rasterizer's int32 radii (used as they are) or the boolean mask radii > 0.
        use_absgrad: accumulate the row norms of `viewspace_point_tensor.absgrad` (a frame rendered with absgrad=True, after backward()) instead of those of
        `.grad`: sum_pixels |dL_pixel/dmean2D| does not cancel where a large Gaussian blurs fine texture (AbsGS).  The statistic is larger than the signed one,
        so densify_and_prune wants a larger grad_threshold with it: the threshold stays the caller's."""
        from . import _lib
        if use_absgrad:
            grad = getattr(viewspace_point_tensor, 'absgrad', None)
            if not torch.is_tensor(grad):
                raise RuntimeError('add_densification_stats: use_absgrad=True, but the viewspace tensor carries no .absgrad -- render the frame with absgrad=True '
                                   '(render_image_training(..., absgrad=True)) and call backward() first')
        else:
            grad = viewspace_point_tensor.grad if viewspace_point_tensor.grad is not None else viewspace_point_tensor
        radii = visibility if visibility.dtype == torch.int32 else visibility.to(torch.int32)
        _lib.check_input(grad, 'viewspace gradient', torch.float32)
        _lib.check_input(radii, 'radii', torch.int32)
        lib = _lib.load()
        _lib.check(lib.nrc_gs_densify_stats(_lib.ptr(grad), grad.shape[1], _lib.ptr(radii), grad.shape[0], _lib.ptr(self.densification_gradient_accum),
                                            _lib.ptr(self.n_observations), _lib.stream_of(grad)), 'gs_densify_stats')

    @torch.no_grad()
    def densify_and_prune(self, grad_threshold: float, min_opacity: float, prune_large_gaussians: bool, noise: torch.Tensor | None = None) -> dict[str, int]:
        """Model.py:226-241 (duplicate, split, prune) as one device plan + one gather.  `noise`: optional (>= 2 * n_split, 3) standard
        normal draws; by default torch.randn((2 * n_split, 3)) -- the draws torch.normal(mean=0, std=stds) consumes in the reference
        (normal_(0, 1) into the output, then * std)."""
        from . import _lib
        from .adam_utils import gather_param_groups
        lib = _lib.load()
        P, dev = self._positions.shape[0], self._positions.device
        src = torch.empty(2 * max(P, 1), dtype=torch.int32, device=dev)
        kind, aux = torch.empty_like(src), torch.empty_like(src)
        counts = torch.zeros(5, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.nrc_gs_densify_plan_ws_bytes(P)), dtype=torch.uint8, device=dev)
        scales, opac = self._scales.data.contiguous(), self._opacities.data.contiguous()
        max_scale = float(np.float32(0.1 * self.training_cameras_extent)) if prune_large_gaussians else 0.0
        _lib.check(lib.nrc_gs_densify_plan(_lib.ptr(self.densification_gradient_accum), _lib.ptr(self.n_observations), _lib.ptr(scales), _lib.ptr(opac), P,
                                           grad_threshold, self.percent_dense * self.training_cameras_extent, min_opacity, max_scale, _lib.ptr(src),
                                           _lib.ptr(kind), _lib.ptr(aux), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_of(src)), 'gs_densify_plan')
        n_out, n_keep, n_dup, n_child, n_split = counts.tolist()  # the one host read: sizes of the new tensors
        if noise is None:
            noise = torch.randn((2 * n_split, 3), dtype=torch.float32, device=dev)
        elif noise.shape[0] < 2 * n_split:
            raise RuntimeError(f'densify_and_prune: noise has {noise.shape[0]} rows, {2 * n_split} needed')
        old_pos, old_rot = self._positions.data, self._rotations.data.contiguous()
        new = gather_param_groups(self.optimizer, src, n_out, kind, None, 'extend_param_groups')
        if n_child > 0:
            noise = noise.to(torch.float32).contiguous()
            _lib.check(lib.nrc_gs_densify_split_children(_lib.ptr(src), _lib.ptr(kind), _lib.ptr(aux), n_out, _lib.ptr(old_pos), _lib.ptr(scales),
                                                         _lib.ptr(old_rot), _lib.ptr(noise), _lib.ptr(new['positions'].data), _lib.ptr(new['scales'].data),
                                                         _lib.stream_of(src)), 'gs_densify_split_children')
        self._adopt(new)
        self.densification_gradient_accum = torch.zeros((n_out, 1), dtype=torch.float32, device=dev)
        self.n_observations = torch.zeros((n_out, 1), dtype=torch.int32, device=dev)
        return {'n_out': n_out, 'n_kept': n_keep, 'n_cloned': n_dup, 'n_split': n_split, 'n_children_kept': 2 * n_child}

    # ---------------------------------------------------------------- 3DGS-MCMC (include/nerficg_hip.h group 16)
    def _six(self) -> list[torch.Tensor]:
        return [getattr(self, attr) for attr in self._GROUP_OF.values()]

    def _adam_moments(self) -> list[torch.Tensor]:
        """Both Adam moments of the six groups (those the optimizer has created so far)."""
        out = []
        if self.optimizer is not None:
            for p in self._six():
                state = self.optimizer.state.get(p) or {}
                out += [state[key] for key in ('exp_avg', 'exp_avg_sq') if key in state]
        return out

    def _drop_grads(self) -> None:
        for p in self._six():
            p.grad = None

    @torch.no_grad()
    def relocate(self, min_opacity: float = 0.005, sampled: torch.Tensor | None = None) -> dict[str, int]:
        """The relocation round of 3DGS-MCMC: every dead Gaussian (o <= min_opacity) is moved onto a live one, drawn with replacement with probability
        o / (sum o + 2^-23) (torch.multinomial); a live Gaussian drawn `count` times becomes one of count + 1 stacked copies with the opacity and scale
        that keep the rendered result (nrc_gs_mcmc_relocation, f64 inside) and loses its Adam moments; the six parameter rows drawn[j] are then copied
        to dead[j], which keep their own moments (as published).  `sampled`: the drawn rows (n_dead indices of live rows) instead of the draw -- the
        test hook that `noise=` is for densify_and_prune.  When a row moved, the .grad of the six tensors is dropped: that iteration's optimizer step
        is skipped, as it is behind densify_and_prune (rest_step_schedule).  Returns {'n_dead', 'n_relocated'}."""
        from . import adam_utils
        o = torch.sigmoid(self._opacities.data).reshape(-1)
        P = o.shape[0]
        dead_mask = o <= min_opacity
        dead = torch.nonzero(dead_mask).reshape(-1)
        n_dead = int(dead.numel())
        if n_dead == 0 or n_dead == P:      # nothing to move, or nothing to move onto
            return {'n_dead': n_dead, 'n_relocated': 0}
        if sampled is None:
            alive = torch.nonzero(~dead_mask).reshape(-1)
            weights = o[alive]
            drawn = alive[_mcmc_draw(weights / (weights.sum() + 2.0 ** -23), n_dead)]
        else:
            drawn = sampled.to(device=o.device, dtype=torch.int64).reshape(-1)
            if drawn.numel() != n_dead or bool(dead_mask[drawn].any()):
                raise RuntimeError(f'relocate: sampled must hold {n_dead} indices of live rows')
        counts = torch.bincount(drawn, minlength=P).to(torch.int32)
        _mcmc_relocation(self._opacities.data, self._scales.data, counts, self._adam_moments())
        tensors = [p.data for p in self._six()]
        rows = adam_utils.gather_rows(tensors, drawn.to(torch.int32), n_dead)
        adam_utils.scatter_rows(rows, tensors, dead.to(torch.int32))
        self._drop_grads()
        self.filter_3D = None   # rows moved: the caller computes the 3-D filter again
        return {'n_dead': n_dead, 'n_relocated': n_dead}

    @torch.no_grad()
    def add_new(self, cap_max: int, sampled: torch.Tensor | None = None) -> int:
        """The growth step of 3DGS-MCMC: n = max(0, min(cap_max, int(1.05 P)) - P) rows are drawn from ALL rows with probability o / (sum o + 2^-23); the
        drawn rows get the relocation arithmetic in place (moments cleared) and one copy per draw is appended with zero moments.  `sampled`: the n drawn
        rows instead of the draw.  The six tensors are replaced by fresh Parameters without .grad (that iteration's optimizer step is skipped);
        densification_gradient_accum / n_observations grow by zero rows.  Returns n."""
        from . import adam_utils
        P = self._positions.shape[0]
        n = max(0, min(int(cap_max), int(1.05 * P)) - P)
        if n == 0:
            return 0
        o = torch.sigmoid(self._opacities.data).reshape(-1)
        if sampled is None:
            drawn = _mcmc_draw(o / (o.sum() + 2.0 ** -23), n)
        else:
            drawn = sampled.to(device=o.device, dtype=torch.int64).reshape(-1)
            if drawn.numel() != n:
                raise RuntimeError(f'add_new: sampled must hold {n} row indices')
        counts = torch.bincount(drawn, minlength=P).to(torch.int32)
        _mcmc_relocation(self._opacities.data, self._scales.data, counts, self._adam_moments())
        src = torch.cat([torch.arange(P, dtype=torch.int32, device=o.device), drawn.to(torch.int32)])
        kind = torch.cat([torch.zeros(P, dtype=torch.int32, device=o.device), torch.ones(n, dtype=torch.int32, device=o.device)])
        self._adopt(adam_utils.gather_param_groups(self.optimizer, src, P + n, kind, None, 'extend_param_groups'))
        self.densification_gradient_accum = torch.cat([self.densification_gradient_accum, self.densification_gradient_accum.new_zeros((n, 1))])
        self.n_observations = torch.cat([self.n_observations, self.n_observations.new_zeros((n, 1))])
        return n

    @torch.no_grad()
    def inject_noise(self, iteration: int | None, noise_lr: float = 5e5, seed: int = 0, z: torch.Tensor | None = None, z_out: torch.Tensor | None = None) -> None:
        """The SGLD noise of 3DGS-MCMC on the positions, after optimizer.step(): x += R diag(s^2) R^T (z * gate * noise_lr * lr), lr the learning rate of
        the `positions` group, gate = sigmoid(100 ((1 - o) - 0.995)) (one streaming launch: nrc_gs_mcmc_noise).  `z`: the caller's (P, 3) standard normal
        draw; by default the kernel draws (Philox4x32-10 keyed by seed, counter = (row, iteration): the same draw on every rank of a view-parallel run).
        z_out: (P, 3), receives the draw that was used.  iteration=None with a capturable optimizer: generator and learning rate are keyed by the
        optimizer's own device scalars (the step counter of the `positions` group), so a step recorded in a HIP graph draws anew on every replay."""
        gi, group = next((i, g) for i, g in enumerate(self.optimizer.param_groups) if g.get('name') == 'positions')
        lr_dev = device_step = None
        if iteration is None:
            slot = getattr(self.optimizer, '_lr_dev', {}).get(gi)
            if not getattr(self.optimizer, 'capturable', False) or slot is None or not torch.is_tensor(group.get('step')):
                raise RuntimeError('inject_noise: iteration=None needs a capturable optimizer that has taken a step (its device step counter keys the generator)')
            lr_dev, device_step, iteration = slot[0], group['step'], 0
        mcmc_noise(self._positions.data, self._rotations.data, self._scales.data, self._opacities.data, float(group['lr']), noise_lr=noise_lr, seed=seed,
                   iteration=iteration, z=z, z_out=z_out, lr_dev=lr_dev, device_step=device_step)

    @torch.no_grad()
    def add_mcmc_regulariser_grads(self, opacity_reg: float = 0.01, scale_reg: float = 0.01) -> tuple[torch.Tensor, torch.Tensor]:
        """The two L1 regularisers of 3DGS-MCMC, L_o = opacity_reg * mean(o) and L_s = scale_reg * mean(s): their gradients are added in place to the .grad
        the backward pass left on the opacity and scale tensors (created as zeros where there is none), the two loss values come back as device scalars
        (bit-reproducible: nrc_gs_mcmc_regularise)."""
        for p in (self._opacities, self._scales):
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
        losses = mcmc_regulariser_grads(self._opacities.data, self._scales.data, self._opacities.grad, self._scales.grad, opacity_reg, scale_reg)
        return losses[0], losses[1]

    # ---------------------------------------------------------------- export (Model.py:248-318)
    @torch.no_grad()
    def bake_activations(self) -> None:
        """Model.py:248-273: activations folded into the parameters, never-visible Gaussians pruned, Morton order, covariances baked."""
        from .adam_utils import compact_mask, gather_rows
        from .MortonEncoding import morton_encode
        rot, opa, sca = self.get_rotations, self.get_opacities, self.get_scales
        keep = compact_mask(~(opa.flatten() < 0.00392156862))
        names = ('_positions', '_rotations', '_features_dc', '_features_rest', '_scales', '_opacities')
        vals = gather_rows([self._positions.data, rot.contiguous(), self._features_dc.data, self._features_rest.data, sca.contiguous(), opa.contiguous()],
                           keep, keep.numel())
        order = torch.argsort(morton_encode(vals[0])).to(torch.int32)
        vals = gather_rows(vals, order, order.numel())
        for name, v in zip(names, vals):
            setattr(self, name, torch.nn.Parameter(v, requires_grad=getattr(self, name).requires_grad))
        self.baked = True
        self._baked_covariances = torch.nn.Parameter(self.get_covariances(1.0), requires_grad=False)

    @torch.no_grad()
    def as_ply_dict(self) -> dict[str, np.ndarray]:
        """The 'vertex' element of the standard 3DGS .ply (Model.py:275-318): every property f4 -- x y z, f_dc_0..2, f_rest_0.. (channel-major),
        opacity (logit), scale_0..2 (log), rot_0..3 (unit quaternion)."""
        n = self._positions.shape[0]
        if n == 0:
            return {}
        channel_major = lambda t: t.detach().permute(0, 2, 1).reshape(n, -1)
        columns = {'x y z': self._positions.detach(), 'f_dc': channel_major(self._features_dc), 'f_rest': channel_major(self._features_rest),
                   'opacity': torch.special.logit(self.get_opacities).detach(), 'scale': torch.log(self.get_scales).detach(), 'rot': self.get_rotations.detach()}
        names: list[str] = []
        for key, block in columns.items():
            width = block.shape[1]
            names += key.split() if ' ' in key else ([key] if (width == 1 and key == 'opacity') else [f'{key}_{i}' for i in range(width)])
        table = torch.cat([block.reshape(n, -1).float() for block in columns.values()], dim=1).cpu().numpy()
        vertex = np.empty(n, dtype=[(name, 'f4') for name in names])
        for column, name in enumerate(names):
            vertex[name] = table[:, column]
        return {'vertex': vertex}


def rest_step_schedule(densify_start_iteration: int, densify_end_iteration: int, densification_interval: int):
    """iteration -> may the f_rest optimizer step of that iteration run inside the backward pass (Gaussians.fuse_rest_step) without leaving the reference's trajectory?

    The reference's trainer runs `densify` (priority 90) between `loss.backward()` (priority 100) and `optimizer.step()` (priority 70), Trainer.py:76-128.  A callback
    fires when start <= iteration <= end and (iteration - start) % stride == 0 (Base/Trainer.py:238-243); `densify` returns at once in its first and last iteration
    (Trainer.py:104-105) and otherwise calls densify_and_prune, whose prune_points replaces ALL six parameter tensors by fresh nn.Parameters without .grad
    (Model.py:157-167, 242-252): the optimizer then finds no gradient and that iteration's update is dropped.  A step applied inside the backward pass has already
    happened by then, so those iterations keep the plain order.  `reset_opacities` (priority 80) replaces the opacity tensor only: the f_rest step is not affected.
    Install with `gaussians.fuse_rest_schedule = rest_step_schedule(DENSIFY_START_ITERATION, DENSIFY_END_ITERATION, DENSIFICATION_INTERVAL)`; the trainer's own
    `update_learning_rate(iteration + 1)` call then sets `fuse_rest_step` for the iteration."""
    a, b, k = int(densify_start_iteration), int(densify_end_iteration), int(densification_interval)
    if k <= 0:
        raise ValueError('densification_interval must be positive')

    def clean(iteration: int) -> bool:
        return not (a < iteration < b and (iteration - a) % k == 0)
    return clean


class RestStep:
    """The optimizer step of the model's `f_rest` group, handed to the rasterizer's backward pass (which applies it where the gradient rows are: C ABI
    nrc_gs_backward_rest_step).  take() is called once per backward: it advances the group's step counter like FusedAdam.step would (apex: one counter per
    group, advanced whenever the group has gradients) and returns the tensors and host scalars of this step.  The optimizer's own step() then finds no
    gradient on the tensor and leaves it alone.  Plain (non-capturable) FusedAdam only; eps / betas / learning rate as the group has them."""

    def __init__(self, gaussians: 'Gaussians') -> None:
        opt = gaussians.optimizer
        self.opt = opt
        self.group = next(g for g in opt.param_groups if g.get('name') == 'f_rest')
        self.param = self.group['params'][0]
        from .apex_optimizers import FusedAdam
        if not isinstance(opt, FusedAdam) or opt.capturable or self.group.get('weight_decay', 0.0) != 0.0 or opt.adam_w_mode:
            raise RuntimeError('RestStep: a plain (non-capturable) nerficg_amd FusedAdam in L2 mode without weight decay is expected (Model.py:131-136)')

    def take(self):
        g, p = self.group, self.param
        state = self.opt.state[p]
        if len(state) == 0:
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        g['step'] = g.get('step', 0) + 1
        beta1, beta2 = g['betas']
        bc = (1.0 - beta1 ** g['step'], 1.0 - beta2 ** g['step']) if g.get('bias_correction', True) else (1.0, 1.0)
        return p, state['exp_avg'], state['exp_avg_sq'], float(g['lr']), float(beta1), float(beta2), float(g['eps']), bc[0], bc[1]


def render_image_training(gaussians: Gaussians, cam: PerspectiveCamera, c2w: np.ndarray, fuse_rest_step: bool | None = None,
                          band: tuple[int, int] | None = None, depth_alpha: bool = False, camera_grad: bool | None = None,
                          features: torch.Tensor | None = None, absgrad: bool = False, antialiasing: bool = False) -> dict[str, torch.Tensor]:
    """GaussianSplatting/Renderer.py:51-86.  antialiasing: anti-aliased splats (the rasterizer's `antialiasing`: the blended opacity is o * comp); the backward
    that steps f_rest has no anti-aliased form: fuse_rest_step=None then resolves to "not fused", an explicit fuse_rest_step=True raises (RuntimeError), and
    camera_grad is refused with it.  A model whose filter_3D is set (Gaussians.compute_3d_filter) is rendered with get_scales_with_3d_filter and
    get_opacities_with_3d_filter through the activated-value path (autograd carries the gradients to the raw tensors; no fused f_rest step then either); a
    filter of another length than the model raises.  absgrad: after backward() outputs['viewspace_points'].absgrad holds sum_pixels |dL_pixel/dmean2D| per Gaussian, (P, 3)
    with column 2 zero (the rasterizer's `absgrad`; Gaussians.add_densification_stats(..., use_absgrad=True) reads it).  The backward that steps f_rest has no
    absgrad form: fuse_rest_step=None then resolves to "not fused", an explicit fuse_rest_step=True raises (RuntimeError).  The same holds for a model set up with
    training_setup(sparse_adam=True): the in-backward f_rest step is dense over all rows, the masked step is Gaussians.optimizer_step(radii).  features: a (P, C) float32 tensor of the caller's (it is NOT carried through densification: the caller owns it); the
    outputs gain 'features', (C, H, W), blended with the colour's weights and differentiable to the tensor and the geometry (the rasterizer's `features`) -- refused
    together with the fused f_rest step (RuntimeError), like depth_alpha.  camera_grad (default None: on exactly when `c2w` is a tensor that requires grad): the loss is differentiated with
    respect to the pose as well (the rasterizer's `camera_grad`; pose refinement, tracking against a frozen model) -- refused together with the fused f_rest step
    (RuntimeError), like a band.  depth_alpha: the outputs gain 'alpha' and 'depth', (1, H, W) like 'rgb' is (3, H, W), both differentiable: alpha = 1 - T of
    the blend, depth = (sum w z) / (alpha + 1e-6), the normalisation of InstantNGP/Renderer.py:82 (the rasterizer's `return_depth_alpha`).  Refused together with the
    fused f_rest step (RuntimeError), like a band.  band = (tile_row_begin, n_tile_rows): this call renders and differentiates that band of 16-pixel tile rows of
    the frame only (the rasterizer's `tile_rows`; parallel.tile_row_band): 'rgb' is zero outside the band, the gradients are the band's share, and the
    outputs gain 'band_mask' (the Gaussians that can receive a gradient from the band).  A band holds a partial gradient, so the in-backward optimizer
    step of `f_rest` is refused with it (RuntimeError), whether asked for here or through gaussians.fuse_rest_step.  fuse_rest_step (default: gaussians.fuse_rest_step, False unless set): the backward pass of this frame applies the
    optimizer's step to the `f_rest` SH tensor itself -- for loops that run exactly one backward pass and one optimizer.step() per frame on one GPU (the
    view-parallel exchange needs the gradient on the wire, gradient accumulation needs it in .grad: both leave this off)."""
    from .diff_gaussian_rasterization import GaussianRasterizer, check_tile_rows, last_band_mask
    positions = gaussians.get_positions
    band = check_tile_rows(band, cam.height)
    fuse = getattr(gaussians, 'fuse_rest_step', False) if fuse_rest_step is None else bool(fuse_rest_step)
    if getattr(gaussians, 'sparse_adam', False):
        if fuse_rest_step is not None and fuse:
            raise RuntimeError('render_image_training: fuse_rest_step=True on a model set up with sparse_adam -- the backward pass that steps f_rest steps every row, '
                               'invisible ones included (a zero gradient still decays their moments); the masked step is optimizer_step(radii), leave fuse_rest_step off')
        fuse = False
    absgrad = bool(absgrad)
    if absgrad:
        if fuse_rest_step is not None and fuse:
            raise RuntimeError('render_image_training: absgrad= together with the fused f_rest step -- the backward pass that steps f_rest takes the colour '
                               'gradient only (the rasterizer refuses absgrad with rest_step); leave fuse_rest_step off for frames that collect the abs-gradient')
        fuse = False
    antialiasing = bool(antialiasing)
    if antialiasing:
        if fuse_rest_step is not None and fuse:
            raise RuntimeError('render_image_training: antialiasing= together with the fused f_rest step -- the backward pass that steps f_rest has no anti-aliased '
                               'form (the rasterizer refuses antialiasing with rest_step); leave fuse_rest_step off for anti-aliased frames')
        fuse = False
    filtered = getattr(gaussians, 'filter_3D', None) is not None
    if filtered:
        if fuse_rest_step is not None and fuse:
            raise RuntimeError('render_image_training: fuse_rest_step=True on a model with a 3-D filter -- the filtered scales and opacities go through the '
                               'activated-value path, which has no in-backward f_rest step; leave fuse_rest_step off')
        fuse = False
    if band is not None and fuse:
        raise RuntimeError('render_image_training: band= together with the fused f_rest step -- the backward pass of a band holds that band\'s share of the '
                           'gradient only, and Adam applied to a partial gradient is not the optimizer\'s step; sum the shares over the bands and step then')
    camera_grad = bool(torch.is_tensor(c2w) and c2w.requires_grad) if camera_grad is None else bool(camera_grad)
    if camera_grad and fuse:
        raise RuntimeError('render_image_training: camera_grad together with the fused f_rest step -- the backward pass that steps f_rest has no camera gradient '
                           '(the rasterizer refuses camera_grad with rest_step); leave fuse_rest_step off for frames whose pose is optimised')
    if depth_alpha and fuse:
        raise RuntimeError('render_image_training: depth_alpha= together with the fused f_rest step -- the backward pass that steps f_rest takes the colour '
                           'gradient only (the rasterizer refuses return_depth_alpha with rest_step); leave fuse_rest_step off for frames with a depth or alpha loss')
    if features is not None and fuse:
        raise RuntimeError('render_image_training: features= together with the fused f_rest step -- the backward pass that steps f_rest takes the colour '
                           'gradient only (the rasterizer refuses features with rest_step); leave fuse_rest_step off for frames with a feature loss')
    # the carrier of the screen-space gradient (Renderer.py:56-58: zeros_like + 0, retain_grad): the rasterizer never reads its VALUES, only hands it a
    # gradient -- a leaf of uninitialised memory receives the same .grad without a 12 MB fill and a 24 MB add per step
    viewspace_points = torch.empty_like(positions).requires_grad_(True)
    rasterizer = GaussianRasterizer(make_raster_settings(cam, c2w, gaussians.active_sh_degree, 1.0, positions.device))
    if filtered:  # the 3-D filter's activations are plain torch on top of the model's own: activated values into the kernels
        image, radii, *aux = rasterizer(means3D=positions, means2D=viewspace_points, shs=gaussians.get_features_dc, shs_rest=gaussians.get_features_rest,
                                        opacities=gaussians.get_opacities_with_3d_filter, scales=gaussians.get_scales_with_3d_filter, rotations=gaussians.get_rotations,
                                        tile_rows=band, return_depth_alpha=depth_alpha, camera_grad=camera_grad, features=features, absgrad=absgrad,
                                        antialiasing=antialiasing)
    elif gaussians.baked:  # a baked model holds activated values
        image, radii, *aux = rasterizer(means3D=positions, means2D=viewspace_points, shs=gaussians.get_features_dc, shs_rest=gaussians.get_features_rest,
                                        opacities=gaussians.get_opacities, scales=gaussians.get_scales, rotations=gaussians.get_rotations, tile_rows=band,
                                        return_depth_alpha=depth_alpha, camera_grad=camera_grad, features=features, absgrad=absgrad, antialiasing=antialiasing)
    else:  # raw parameters straight into the kernels: no get_features concatenation, no separate exp / sigmoid / normalize passes (a25)
        rest_step = RestStep(gaussians) if fuse and not getattr(gaussians.optimizer, 'capturable', False) and not torch.cuda.is_current_stream_capturing() and torch.is_grad_enabled() and gaussians._features_rest.requires_grad and gaussians._features_rest.shape[1] > 0 and torch.is_tensor(c2w) else None
        image, radii, *aux = rasterizer(means3D=positions, means2D=viewspace_points, shs=gaussians._features_dc, shs_rest=gaussians._features_rest,
                                        opacities=gaussians._opacities, scales=gaussians._scales, rotations=gaussians._rotations, raw_parameters=True, rest_step=rest_step,
                                        tile_rows=band, return_depth_alpha=depth_alpha, camera_grad=camera_grad, features=features, absgrad=absgrad,
                                        antialiasing=antialiasing)
    outputs = _TrainingOutputs({'rgb': image, 'viewspace_points': viewspace_points, 'radii': radii})
    if depth_alpha:
        outputs.update(_depth_alpha_outputs(aux[0], aux[1], True))
    if features is not None:
        outputs['features'] = aux[-1]
    if band is not None:
        outputs['band_mask'] = last_band_mask()
    return outputs


def band_parallel_training_step(gaussians: Gaussians, cam: PerspectiveCamera, c2w, loss_fn, exchange=None, rank: int | None = None,
                                world: int | None = None, antialiasing: bool = False) -> dict[str, torch.Tensor]:
    """The training render of ONE view split over the ranks as bands of tile rows, forward and backward, with the reference's one-view semantics:

        1. this rank renders its own band (parallel.tile_row_band of the frame's ceil(H / 16) tile rows);
        2. the band images are gathered: every rank holds the whole frame, bit for bit the single-GPU image (parallel.gather_band_images);
        3. `loss_fn(image)` -- the caller's usual loss on the WHOLE (3, H, W) frame, the same value on every rank (SSIM windows need no halo logic);
        4. backward: each rank receives its own rows of the image gradient and computes its band's share of every parameter gradient;
        5. the shares are SUMMED (not averaged) over the ranks -- the six model tensors and the screen-space gradient of 'viewspace_points' that
           densification reads -- through parallel.UnionRowExchange with the band mask as `visible`: only rows that some band touches travel.

    Afterwards every rank holds the single-GPU gradient and takes the single-GPU optimizer step: preprocess, depth sort, per-Gaussian backward and
    Adam are replicated, binning and the two blend kernels shrink with the band.  Returns the outputs of render_image_training with 'rgb' = the whole
    frame (detached), plus 'loss' and 'band'.  `exchange`: a parallel.UnionRowExchange(P, device) to reuse across steps of the same P.
    The in-backward f_rest step (gaussians.fuse_rest_step) is refused: it would run on a partial gradient.  antialiasing: passed to render_image_training."""
    from . import parallel
    r, w = parallel.world_info()
    rank, world = (r if rank is None else int(rank)), (w if world is None else int(world))
    band = parallel.tile_row_band((cam.height + 15) // 16, rank, world)
    out = render_image_training(gaussians, cam, c2w, band=band, antialiasing=antialiasing)
    mask = out['band_mask']
    ex = exchange if exchange is not None else parallel.UnionRowExchange(mask.shape[0], mask.device)
    ex.begin(mask)          # the mask traffic runs beside the gather, the loss and the backward pass
    image = parallel.gather_band_images(out['rgb'], rank, world)
    loss = loss_fn(image)
    loss.backward()
    carriers = [gaussians._positions, gaussians._features_dc, gaussians._features_rest, gaussians._opacities, gaussians._scales, gaussians._rotations,
                out['viewspace_points']]
    ex.finish([p for p in carriers if p.requires_grad], average=False)
    out['rgb'], out['loss'], out['band'] = image.detach(), loss.detach(), band
    return out


def _depth_alpha_outputs(depth_sum: torch.Tensor, alpha: torch.Tensor, to_chw: bool) -> dict[str, torch.Tensor]:
    """'alpha' and 'depth' of a frame from the rasterizer's (H, W) maps, laid out like instant_ngp.render_image lays them out: (H, W, 1), or (1, H, W) with
    to_chw; depth normalised as InstantNGP/Renderer.py:82 does, depth / (alpha + 1e-6)."""
    depth = depth_sum / (alpha + 1e-6)
    if to_chw:
        return {'alpha': alpha[None], 'depth': depth[None]}
    return {'alpha': alpha[..., None], 'depth': depth[..., None]}


class _TrainingOutputs(dict):
    """The outputs of Renderer.py:83-86; 'visibility_mask' (radii > 0) is built when somebody asks for it -- the densification statistics and the view-parallel
    exchange take `radii` itself, so the plain step does not pay the launch."""

    def __missing__(self, key):
        if key == 'visibility_mask':
            self[key] = self['radii'] > 0
            return self[key]
        raise KeyError(key)

    def __contains__(self, key):
        return key == 'visibility_mask' or super().__contains__(key)


@torch.no_grad()
def render_image_inference(gaussians: Gaussians, cam: PerspectiveCamera, c2w: np.ndarray, scale_modifier: float = 1.0, to_chw: bool = False,
                           use_baked_covariance: bool = True, band: tuple[int, int] | None = None, depth_alpha: bool = False,
                           features: torch.Tensor | None = None, _rasterizer_out: list | None = None, antialiasing: bool = False):
    """antialiasing: anti-aliased splats (the rasterizer's `antialiasing`).  A model whose filter_3D is set is rendered with get_scales_with_3d_filter and
    get_opacities_with_3d_filter (not from baked covariances, which do not hold the filter); a filter of another length than the model raises.  features: a (P, C) float32 tensor of the caller's; the outputs gain 'features', the map blended with the colour's weights (the rasterizer's `features`),
    (H, W, C) or (C, H, W) with to_chw.  depth_alpha: the outputs gain 'alpha' (1 - T of the blend) and 'depth' (accumulated view-space depth / (alpha + 1e-6)), (H, W, 1) or (1, H, W) with to_chw, as
    instant_ngp.render_image returns them.  band = (tile_row_begin, n_tile_rows): only that band of tile rows of the frame is rendered (zero elsewhere; parallel.gather_band_images composes the
    frame from the ranks' bands).  GaussianSplatting/Renderer.py:89-155 with the fused SH path (USE_FUSED_SH_CONVERSION = True, the shipped default); a baked model
    (trained checkpoint, Model.py:248-273) is rasterized from its baked covariances like the reference's USE_BAKED_COVARIANCE branch
    (Renderer.py:129-139), everything else through the in-kernel covariance computation."""
    from .diff_gaussian_rasterization import GaussianRasterizer
    positions = gaussians.get_positions
    rasterizer = GaussianRasterizer(make_raster_settings(cam, c2w, gaussians.active_sh_degree, scale_modifier, positions.device))
    filtered = getattr(gaussians, 'filter_3D', None) is not None
    covariances = gaussians.get_baked_covariances if (use_baked_covariance and gaussians.baked and not filtered) else None
    if covariances is not None and covariances.shape[0] != positions.shape[0]:
        covariances = None  # "Baked covariance requested but not available"
    if covariances is not None:
        image, _, *aux = rasterizer(means3D=positions, means2D=torch.empty_like(positions), shs=gaussians.get_features, opacities=gaussians.get_opacities,
                                    cov3D_precomp=covariances, tile_rows=band, return_depth_alpha=depth_alpha, features=features, antialiasing=antialiasing)
    else:
        image, _, *aux = rasterizer(means3D=positions, means2D=torch.empty_like(positions), shs=gaussians.get_features,
                                    opacities=gaussians.get_opacities_with_3d_filter if filtered else gaussians.get_opacities,
                                    scales=gaussians.get_scales_with_3d_filter if filtered else gaussians.get_scales, rotations=gaussians.get_rotations, tile_rows=band,
                                    return_depth_alpha=depth_alpha, features=features, antialiasing=antialiasing)
    image.clamp_(0.0, 1.0)
    outputs = {'rgb': image if to_chw else image.permute(1, 2, 0)}
    if depth_alpha:
        outputs.update(_depth_alpha_outputs(aux[0], aux[1], to_chw))
    if features is not None:
        outputs['features'] = aux[-1] if to_chw else aux[-1].permute(1, 2, 0)
    if _rasterizer_out is not None:   # accumulate_contributions: the object that holds this frame's state
        _rasterizer_out.append(rasterizer)
    return outputs


@torch.no_grad()
def accumulate_contributions(gaussians: Gaussians, views, pixel_weights=None) -> dict:
    """Per-Gaussian contribution statistics over a set of views (GaussianRasterizer.contributions, C ABI group 22), the input of
    Gaussians.prune_by_contribution: every view is rendered through render_image_inference (no autograd state) and scored with one more launch.
    views: an iterable of (cam, c2w).  pixel_weights: None (every pixel counts 1), a sequence with one (H, W) float32 map per view, or a callable
    (image (3, H, W), index) -> map, e.g. a per-pixel error against the view's target; a pixel whose weight is 0 does not take part.
    Returns {'weight_sum', 'weight_max' (P,) float32, 'hits' (P,) int32, 'n_views': int}: the sum of m w, the largest blending weight and the number of
    pixels that blended each Gaussian, over all views."""
    stats, n_views = None, 0
    for index, (cam, c2w) in enumerate(views):
        holder: list = []
        image = render_image_inference(gaussians, cam, c2w, to_chw=True, _rasterizer_out=holder)['rgb']
        if callable(pixel_weights):
            m = pixel_weights(image, index)
        else:
            m = None if pixel_weights is None else pixel_weights[index]
        stats = holder[0].contributions(m, out=stats)
        holder[0].release_state()
        n_views += 1
    if stats is None:
        P, dev = gaussians.get_positions.shape[0], gaussians.get_positions.device
        stats = dict(weight_sum=torch.zeros(P, device=dev), weight_max=torch.zeros(P, device=dev), hits=torch.zeros(P, dtype=torch.int32, device=dev))
    stats['n_views'] = n_views
    return stats


FUSED_PHOTOMETRIC_LOSS = True   # training_loss as one node (nerficg_amd.fused_ssim.photometric_loss); False: l1_loss + fused_ssim as tensor operations


def training_loss(image: torch.Tensor, target: torch.Tensor, lambda_l1: float = 0.8, lambda_dssim: float = 0.2, depth: torch.Tensor | None = None,
                  alpha: torch.Tensor | None = None, lambda_smooth: float = 0.0, lambda_entropy: float = 0.0, entropy_symmetrical: bool = False) -> torch.Tensor:
    """GaussianSplattingLoss (src/Methods/GaussianSplatting/Loss.py:11-23, weights Trainer.py:34-35): lambda_l1 * L1 + lambda_dssim *
    (1 - SSIM) on (3, H, W) images, SSIM through the HIP kernels (nerficg_amd.fused_ssim; DSSIM.py:11-18 adds the batch dimension).

    lambda_smooth / lambda_entropy (both 0 by default: the photometric loss alone, unchanged) add the map regularisers of nerficg_amd.map_losses as one more
    node: lambda_smooth * depth_smoothness_loss(depth / (alpha + 1e-6), image) + lambda_entropy * background_entropy(alpha, entropy_symmetrical)
    (src/Optim/Losses/DepthSmoothness.py:31-43, BackgroundEntropy.py:6-8).  `depth` is the rasterizer's ACCUMULATED depth (sum w z), NOT the normalised
    'depth' of render_image_training(..., depth_alpha=True): the kernel divides by alpha + 1e-6 itself, so the normalisation costs no launch and its
    gradient reaches both maps.  The raw maps come from the rasterizer call:

        image, radii, depth_sum, alpha = rasterizer(means3D=..., ..., return_depth_alpha=True)        # (3, H, W), (P,), (H, W), (H, W)
        loss = training_loss(image, target, depth=depth_sum, alpha=alpha, lambda_smooth=0.1, lambda_entropy=0.01)

    The image gradient of the smoothness weights flows into `image` as in the reference.  CPU tensors and other dtypes take the tensor formula."""
    from .fused_ssim import fused_ssim, photometric_loss
    a = image[None] if image.dim() == 3 else image
    b = target[None] if target.dim() == 3 else target
    if FUSED_PHOTOMETRIC_LOSS and a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 4 and a.shape == b.shape:
        # one autograd node, three launches (stencil + reduction, stencil) instead of ~22 tensor operations around the SSIM kernels
        loss = photometric_loss(a.contiguous(), b.contiguous(), lambda_l1, lambda_dssim)
    else:
        l1 = torch.nn.functional.l1_loss(image, target)
        loss = lambda_l1 * l1 + lambda_dssim * (1.0 - fused_ssim(a, b))
    if lambda_smooth == 0.0 and lambda_entropy == 0.0:
        return loss
    from .map_losses import map_regularizer
    if alpha is None or (lambda_smooth != 0.0 and depth is None):
        raise RuntimeError('training_loss: lambda_smooth needs depth= and alpha= (the rasterizer\'s return_depth_alpha maps), lambda_entropy needs alpha=')
    return loss + map_regularizer(depth, alpha, a, lambda_smooth, lambda_entropy, normalize=True, symmetrical=entropy_symmetrical)
