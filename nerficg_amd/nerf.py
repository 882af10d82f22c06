"""nerficg_amd.nerf -- host-side mirror of the reference's vanilla NeRF hot path (config 1: nerf_lego.yaml, pure PyTorch, runs
on CPU or on the GPU through torch): FrequencyEncoding, NeRFBlock, stratified + PDF sampling, sample integration and the
hierarchical (coarse -> fine) ray renderer.  `fused_forward` / `render_rays(fused=True)` run the block's INFERENCE forward as one HIP kernel
(csrc/nerf_net.hip, header group 17: fp16 MFMA operands, f32 accumulation).  `fused_apply` / `render_rays(fused_train=True)` are the opt-in TRAINING
path: a forward that keeps every stage's fp16 operand and a backward through the whole block (csrc/nerf_grad.hip, header group 18) behind an autograd
function that returns gradients for the block's parameters; sampling, sorting and compositing stay torch autograd.  `sample_coarse`, `composite`,
`sample_fine` / `render_rays(device_rays=True)` are the opt-in device path for what surrounds the block: stratified sampling, compositing with its
backward and the fine pass's resampling + sorted union as one HIP kernel each (csrc/nerf_rays.hip, header group 19).  `input_grad=True` on any of them (and on
`render_rays`) is the opt-in for gradients to the INPUTS on that device path -- sample positions and viewing directions through the block
(csrc/nerf_input_grad.hip), ray origins and directions through `o + d t` and the compositor's segment lengths (header group 20): pose refinement and
tracking against a frozen model without leaving the fused path.  Everything else stays on torch.

Reference: src/Methods/NeRF/utils.py:12-136, src/Methods/NeRF/Model.py:10-83, src/Methods/NeRF/Renderer.py:20-95.
Pinned against golden vectors generated from the reference (tests/test_host_golden.py).  `integrate_samples` is also the
independent statement of the compositing math that pins oracle/ngp_oracle.c (tests/test_oracle_ngp.py).
"""
from __future__ import annotations

import torch

__all__ = ['FrequencyEncoding', 'NeRFBlock', 'generate_samples', 'generate_samples_from_pdf', 'integrate_samples', 'render_rays', 'fused_forward',
           'fused_config', 'fused_tap_names', 'fused_apply', 'fused_grad_stats', 'sample_coarse', 'sample_fine', 'composite']


class FrequencyEncoding(torch.nn.Module):
    """[x, cos(x 2^k), sin(x 2^k)] for k < K, cos block before sin block per input dimension, no pi factor (utils.py:12-36)."""

    def __init__(self, n_frequencies: int, append_input: bool) -> None:
        super().__init__()
        self.register_buffer('frequency_factors', torch.linspace(0.0, n_frequencies - 1.0, n_frequencies).exp2()[None, None, :])
        self.append_input = append_input

    def get_n_outputs(self, n_inputs: int) -> int:
        return n_inputs * 2 * self.frequency_factors.numel() + (n_inputs if self.append_input else 0)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        f = inputs[..., None] * self.frequency_factors
        enc = torch.cat((torch.cos(f), torch.sin(f)), dim=-1).flatten(start_dim=1)
        return torch.cat([inputs, enc], dim=-1) if self.append_input else enc


class NeRFBlock(torch.nn.Module):
    """8 x (Linear 256 + ReLU) with the encoded position re-appended after layer 5, density head (Linear + ReLU), feature layer,
    colour head on [features, encoded direction] (Model.py:10-83).  Module / parameter names match the reference's state_dict."""

    def __init__(self, n_layers: int = 8, n_color_layers: int = 1, n_features: int = 256, n_frequencies_position: int = 10,
                 n_frequencies_direction: int = 4, encoding_append_input: bool = True, input_skips=(5,)) -> None:
        super().__init__()
        self.input_skips = list(input_skips)
        self.encoding_position = FrequencyEncoding(n_frequencies_position, encoding_append_input)
        self.encoding_direction = FrequencyEncoding(n_frequencies_direction, encoding_append_input)
        n_pos, n_dir = self.encoding_position.get_n_outputs(3), self.encoding_direction.get_n_outputs(3)
        nn = torch.nn
        widths_in = [n_pos] + [n_features + (n_pos if k in self.input_skips else 0) for k in range(1, n_layers)]
        self.initial_layers = nn.ModuleList(nn.Sequential(nn.Linear(w, n_features), nn.ReLU(True)) for w in widths_in)
        self.feature_layer = torch.nn.Linear(n_features, n_features)
        self.density_layer = torch.nn.Linear(n_features, 1)
        self.density_activation = torch.nn.ReLU(True)
        half = n_features // 2
        color = [torch.nn.Linear(n_features + n_dir, half), torch.nn.ReLU(True)]
        color += [torch.nn.Sequential(torch.nn.Linear(half, half), torch.nn.ReLU(True)) for _ in range(n_color_layers - 1)]
        color += [torch.nn.Linear(half, 3), torch.nn.Sigmoid()]
        self.color_layers = torch.nn.Sequential(*color)

    def forward(self, positions: torch.Tensor, directions: torch.Tensor, random_noise_density: float = 0.0):
        encoded = self.encoding_position(positions)
        hidden = encoded
        for depth_index, block in enumerate(self.initial_layers, start=1):
            hidden = block(hidden)
            if depth_index in self.input_skips:  # the encoded position re-enters behind this layer
                hidden = torch.cat((hidden, encoded), dim=-1)
        sigma = self.density_layer(hidden)
        if random_noise_density > 0.0:
            sigma = sigma + torch.randn_like(sigma) * random_noise_density
        view_dependent = torch.cat((self.feature_layer(hidden), self.encoding_direction(directions)), dim=-1)
        return self.density_activation(sigma), self.color_layers(view_dependent)


def _block_linears(block: NeRFBlock) -> list:
    """The block's linears in the order of the packed parameter list (include/nerficg_hip.h group 17)."""
    color = list(block.color_layers)
    return ([seq[0] for seq in block.initial_layers] + [block.density_layer, block.feature_layer, color[0]] + [m[0] for m in color[2:-2]] + [color[-2]])


def fused_config(block: NeRFBlock):
    """(width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask) of a block the fused kernel can
    run (nrc_nerf_supported), None for any other: widths other than 128 / 256, encodings wider than 64 / 32, differing append flags, non-f32 parameters."""
    from . import _lib
    n_layers, width = len(block.initial_layers), block.feature_layer.in_features
    skips = {int(k) for k in block.input_skips if 1 <= int(k) <= n_layers}   # the module itself ignores every other entry
    if n_layers in skips or bool(block.encoding_position.append_input) != bool(block.encoding_direction.append_input):
        return None
    cfg = (width, n_layers, len(block.color_layers) - 3, block.encoding_position.frequency_factors.numel(),
           block.encoding_direction.frequency_factors.numel(), int(bool(block.encoding_position.append_input)), sum(1 << k for k in skips))
    if not _lib.load().nrc_nerf_supported(*cfg):
        return None
    n_pos, n_dir, half = block.encoding_position.get_n_outputs(3), block.encoding_direction.get_n_outputs(3), width // 2
    shapes = ([(width, n_pos)] + [(width, width + (n_pos if k in skips else 0)) for k in range(1, n_layers)] + [(1, width), (width, width), (half, width + n_dir)]
              + [(half, half)] * (cfg[2] - 1) + [(3, half)])
    linears = _block_linears(block)
    if len(linears) != len(shapes):
        return None
    for lin, shape in zip(linears, shapes):
        if (not isinstance(lin, torch.nn.Linear) or tuple(lin.weight.shape) != shape or lin.bias is None or lin.weight.dtype != torch.float32
                or lin.bias.dtype != torch.float32 or not lin.weight.is_contiguous()):
            return None
    return cfg


def fused_tap_names(cfg) -> list[tuple[str, int]]:
    """(name, width) of the stages `fused_forward(tap=...)` can return, in the kernel's order; tap = 1 + index."""
    width, n_layers, n_color, k_pos, k_dir, append = cfg[:6]
    return ([('enc_pos', 6 * k_pos + 3 * append), ('enc_dir', 6 * k_dir + 3 * append)] + [(f'H_{l}', width) for l in range(1, n_layers + 1)] + [('F', width)]
            + [(f'C_{q}', width // 2) for q in range(1, n_color + 1)])


def _packed_blob(block: NeRFBlock, cfg, device) -> torch.Tensor:
    """The block's parameters as the kernel's blob, cached on the block; repacked (one launch, no sync) when any parameter's storage or version changed."""
    import ctypes
    from . import _lib
    params = [t for lin in _block_linears(block) for t in (lin.weight, lin.bias)]
    key = (cfg, str(device)) + tuple((t.data_ptr(), t._version) for t in params)
    cache = block.__dict__.setdefault('_fused_cache', {'key': None, 'blob': None, 'packs': 0})
    if cache['key'] != key:
        lib = _lib.load()
        n_bytes = lib.nrc_nerf_packed_bytes(*cfg)
        if cache['blob'] is None or cache['blob'].numel() != n_bytes or cache['blob'].device != device:
            cache['blob'] = torch.empty(n_bytes, dtype=torch.uint8, device=device)
        ptrs = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        _lib.check(lib.nrc_nerf_pack_weights(ctypes.cast(ptrs, ctypes.c_void_p), len(params), *cfg, _lib.ptr(cache['blob']), _lib.stream_of(cache['blob'])),
                   'nerf_pack_weights')
        cache['key'] = key
        cache['packs'] += 1
    return cache['blob']


def fused_forward(block: NeRFBlock, positions: torch.Tensor, directions: torch.Tensor, dir_group: int = 1, tap: int | None = None):
    """`NeRFBlock.forward` without noise as one kernel -> (sigma (M, 1), rgb (M, 3)), f32.  `directions` holds one row per `dir_group` consecutive
    samples (1: per sample; S: per ray of S samples).  With `tap` = t >= 1 a third value is returned: the fp16 operand of stage t of
    `fused_tap_names` (None on the torch path).  Falls back to the torch module -- same values as `block(positions, expanded directions)` -- for CPU
    tensors, an unsupported block, or when autograd is recording and an input or a parameter requires grad."""
    m = positions.shape[0]
    eligible = (positions.is_cuda and directions.is_cuda and positions.dtype == torch.float32 and directions.dtype == torch.float32
                and all(p.is_cuda and p.device == positions.device for p in block.parameters())
                and not (torch.is_grad_enabled() and (positions.requires_grad or directions.requires_grad or any(p.requires_grad for p in block.parameters()))))
    cfg = fused_config(block) if eligible else None
    if cfg is None:
        expanded = directions if dir_group == 1 else directions[:, None, :].expand(-1, dir_group, -1).reshape(-1, 3)[:m]
        out = block(positions, expanded)
        return out if tap is None else (*out, None)
    from . import _lib
    positions, directions = positions.detach().contiguous(), directions.detach().contiguous()
    if directions.shape[0] * dir_group < m:
        raise ValueError(f'{directions.shape[0]} direction rows x dir_group {dir_group} do not cover {m} samples')
    with torch.cuda.device(positions.device):
        blob = _packed_blob(block, cfg, positions.device)
        sigma = torch.empty(m, 1, dtype=torch.float32, device=positions.device)
        rgb = torch.empty(m, 3, dtype=torch.float32, device=positions.device)
        tapped = None
        if tap:
            tapped = torch.empty(m, fused_tap_names(cfg)[tap - 1][1], dtype=torch.float16, device=positions.device)
        _lib.check(_lib.load().nrc_nerf_block_forward(_lib.ptr(positions), _lib.ptr(directions), int(dir_group), m, _lib.ptr(blob), *cfg, _lib.ptr(sigma),
                                                      _lib.ptr(rgb), int(tap or 0), _lib.ptr(tapped), _lib.stream_of(positions)), 'nerf_block_forward')
    return (sigma, rgb) if tap is None else (sigma, rgb, tapped)


def _train_blobs(block: NeRFBlock, cfg, device):
    """(forward blob, transposed blob of the data gradient): the same fp16 values, the second cached under the key of the first."""
    import ctypes
    from . import _lib
    blob = _packed_blob(block, cfg, device)
    cache = block._fused_cache
    if cache.get('key_t') != cache['key']:
        lib = _lib.load()
        n_bytes = lib.nrc_nerf_packed_transposed_bytes(*cfg)
        if cache.get('blob_t') is None or cache['blob_t'].numel() != n_bytes or cache['blob_t'].device != device:
            cache['blob_t'] = torch.empty(n_bytes, dtype=torch.uint8, device=device)
        params = [t for lin in _block_linears(block) for t in (lin.weight, lin.bias)]
        ptrs = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        _lib.check(lib.nrc_nerf_pack_weights_transposed(ctypes.cast(ptrs, ctypes.c_void_p), len(params), *cfg, _lib.ptr(cache['blob_t']),
                                                        _lib.stream_of(cache['blob_t'])), 'nerf_pack_weights_transposed')
        cache['key_t'] = cache['key']
        cache['packs_t'] = cache.get('packs_t', 0) + 1
    return blob, cache['blob_t']


def _input_blob(block: NeRFBlock, cfg, device):
    """The weight stream of the input gradient (header group 20): the same fp16 values again, cached under the key of the forward blob."""
    import ctypes
    from . import _lib
    _packed_blob(block, cfg, device)
    cache = block._fused_cache
    if cache.get('key_i') != cache['key']:
        lib = _lib.load()
        n_bytes = lib.nrc_nerf_packed_input_bytes(*cfg)
        if cache.get('blob_i') is None or cache['blob_i'].numel() != n_bytes or cache['blob_i'].device != device:
            cache['blob_i'] = torch.empty(n_bytes, dtype=torch.uint8, device=device)
        params = [t for lin in _block_linears(block) for t in (lin.weight, lin.bias)]
        ptrs = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        _lib.check(lib.nrc_nerf_pack_weights_input(ctypes.cast(ptrs, ctypes.c_void_p), len(params), *cfg, _lib.ptr(cache['blob_i']),
                                                   _lib.stream_of(cache['blob_i'])), 'nerf_pack_weights_input')
        cache['key_i'] = cache['key']
        cache['packs_i'] = cache.get('packs_i', 0) + 1
    return cache['blob_i']


class _FusedBlock(torch.autograd.Function):
    """Training forward + backward of one block (header group 18).  Gradients for the parameters and -- when the positions or the directions require grad,
    which `fused_apply` lets through only with `input_grad=True` -- for those two (header group 20)."""

    @staticmethod
    def forward(ctx, block, cfg, positions, directions, dir_group, grad_scale, *params):
        from . import _lib
        lib, m, device = _lib.load(), positions.shape[0], positions.device
        with torch.cuda.device(device):
            blob, blob_t = _train_blobs(block, cfg, device)
            cache = block._fused_cache
            n_bytes = lib.nrc_nerf_train_workspace_bytes(*cfg, m)
            pool = cache.setdefault('workspaces', [])        # one per forward whose backward is still to come; grown on demand
            ws = pool.pop() if pool else None
            if ws is None or ws.numel() < n_bytes or ws.device != device:
                ws = torch.empty(n_bytes, dtype=torch.uint8, device=device)
            sigma = torch.empty(m, 1, dtype=torch.float32, device=device)
            rgb = torch.empty(m, 3, dtype=torch.float32, device=device)
            _lib.check(lib.nrc_nerf_block_forward_train(_lib.ptr(positions), _lib.ptr(directions), int(dir_group), m, _lib.ptr(blob), *cfg, _lib.ptr(sigma),
                                                        _lib.ptr(rgb), _lib.ptr(ws), _lib.stream_of(positions)), 'nerf_block_forward_train')
            ctx.blob_i = _input_blob(block, cfg, device) if (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]) else None
        ctx.block, ctx.cfg, ctx.m, ctx.grad_scale, ctx.ws, ctx.blob_t, ctx.dir_group = block, cfg, m, grad_scale, ws, blob_t, int(dir_group)
        if ctx.blob_i is None:
            ctx.save_for_backward(sigma, rgb)
        else:
            ctx.save_for_backward(sigma, rgb, positions, directions)
        return sigma, rgb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_sigma, d_rgb):
        from . import _lib
        lib = _lib.load()
        sigma, rgb = ctx.saved_tensors[:2]
        block, cfg = ctx.block, ctx.cfg
        d_positions = d_directions = None
        d_sigma, d_rgb = d_sigma.contiguous().float(), d_rgb.contiguous().float()
        with torch.cuda.device(sigma.device):
            grad = torch.empty(lib.nrc_nerf_grad_params_floats(*cfg), dtype=torch.float32, device=sigma.device)
            stats = torch.empty(4, dtype=torch.int32, device=sigma.device)
            _lib.check(lib.nrc_nerf_block_backward(_lib.ptr(d_sigma), _lib.ptr(d_rgb), _lib.ptr(sigma), _lib.ptr(rgb), ctx.m, _lib.ptr(ctx.blob_t), *cfg,
                                                   _lib.ptr(ctx.ws), float(ctx.grad_scale or 0.0), _lib.ptr(grad), _lib.ptr(stats), _lib.stream_of(sigma)),
                       'nerf_block_backward')
            if ctx.blob_i is not None:      # before the workspace returns to its pool: the gradient stages are still in it
                positions, directions = ctx.saved_tensors[2:]
                d_positions, d_directions = torch.empty_like(positions), torch.empty_like(directions)
                _lib.check(lib.nrc_nerf_block_input_grad(_lib.ptr(positions), _lib.ptr(directions), ctx.dir_group, ctx.m, _lib.ptr(ctx.blob_i), *cfg,
                                                         _lib.ptr(ctx.ws), float(ctx.grad_scale or 0.0), _lib.ptr(d_positions), _lib.ptr(d_directions), None,
                                                         None, _lib.stream_of(sigma)), 'nerf_block_input_grad')
        cache = block._fused_cache
        cache['stats'], cache['last_workspace'] = stats, ctx.ws
        cache.setdefault('workspaces', []).append(ctx.ws)
        ctx.ws = None
        out, at = [], 0
        for k, lin in enumerate(_block_linears(block)):
            for j, t in enumerate((lin.weight, lin.bias)):
                n = t.numel()
                out.append(grad[at:at + n].view(t.shape) if ctx.needs_input_grad[6 + 2 * k + j] else None)
                at += n
        return (None, None, d_positions if ctx.needs_input_grad[2] else None, d_directions if ctx.needs_input_grad[3] else None, None, None) + tuple(out)


def fused_apply(block: NeRFBlock, positions: torch.Tensor, directions: torch.Tensor, dir_group: int = 1, grad_scale: float | None = None,
                input_grad: bool = False):
    """`NeRFBlock.forward` without noise for TRAINING -> (sigma (M, 1), rgb (M, 3)), f32, differentiable with respect to the block's parameters: the
    forward keeps every stage's fp16 operand, the backward runs the whole block on the matrix units (csrc/nerf_grad.hip) and autograd accumulates
    its result into `.grad` as usual.  `grad_scale`: a positive power of two for the fp16 gradients, None = chosen on the device per call.  Second-order
    gradients are not supported, positions and directions receive none.  Under `torch.no_grad()`, or when no parameter requires grad, this is
    `fused_forward`.  For CPU tensors, a block `nrc_nerf_train_supported` refuses, non-f32 parameters, an empty batch, or positions / directions that
    require grad it returns `block(positions, expanded directions)` with torch's bits and torch's autograd.

    `input_grad=True`: positions or directions that require grad no longer disqualify the call -- the backward also runs the input-gradient kernel
    (csrc/nerf_input_grad.hip, header group 20) and returns their gradients, `directions.grad` summed over the `dir_group` rows that share a row; the
    parameter gradients keep their bits.  The device path then also runs when no parameter requires grad but an input does (tracking against a frozen
    model).  `directions` must then hold exactly ceil(M / dir_group) rows."""
    params = [t for lin in _block_linears(block) for t in (lin.weight, lin.bias)]
    inputs_want = bool(input_grad) and (positions.requires_grad or directions.requires_grad)
    if not torch.is_grad_enabled() or not (any(p.requires_grad for p in block.parameters()) or inputs_want):
        return fused_forward(block, positions, directions, dir_group)
    m = positions.shape[0]
    eligible = (m > 0 and positions.is_cuda and directions.is_cuda and positions.dtype == torch.float32 and directions.dtype == torch.float32
                and all(p.is_cuda and p.device == positions.device for p in block.parameters())
                and (bool(input_grad) or not (positions.requires_grad or directions.requires_grad))
                and not (inputs_want and directions.shape[0] != -(-m // int(dir_group))))
    cfg = fused_config(block) if eligible else None
    if cfg is not None:
        from . import _lib
        if not _lib.load().nrc_nerf_train_supported(*cfg):
            cfg = None
    if cfg is None:
        expanded = directions if dir_group == 1 else directions[:, None, :].expand(-1, dir_group, -1).reshape(-1, 3)[:m]
        return block(positions, expanded)
    if grad_scale is not None:
        import math
        if not (grad_scale > 0.0 and math.frexp(grad_scale)[0] == 0.5 and 2.0 ** -126 <= grad_scale <= 2.0 ** 126):
            raise ValueError(f'grad_scale {grad_scale} is not a positive power of two in [2^-126, 2^126]')
    positions, directions = positions.contiguous(), directions.contiguous()
    if directions.shape[0] * dir_group < m:
        raise ValueError(f'{directions.shape[0]} direction rows x dir_group {dir_group} do not cover {m} samples')
    return _FusedBlock.apply(block, cfg, positions, directions, int(dir_group), grad_scale, *params)


def fused_grad_stats(block: NeRFBlock):
    """The statistics of the block's last fused backward, an int32 tensor ON THE DEVICE (reading it is the caller's synchronisation): [0] the exponent of
    the gradient scale that was used, [1] gradient elements that overflowed fp16 and were saturated at +-65504, [2..3] 0.  None before the first."""
    return block.__dict__.get('_fused_cache', {}).get('stats')


def generate_samples(n_rays: int, n_samples: int, near_plane: float, far_plane: float, randomize_samples: bool, dtype=torch.float32,
                     device=None) -> torch.Tensor:
    """Depths of the coarse pass (utils.py:57-75): `n_samples` evenly spaced values in [near, far] for every ray; with `randomize_samples` each
    one is redrawn uniformly inside its stratum (the strata meet at the mid points, the two outer ones end at near / far)."""
    t = torch.linspace(near_plane, far_plane, n_samples, dtype=dtype, device=device).expand(n_rays, n_samples)
    if not randomize_samples:
        return t
    return _stratified(t, torch.rand(t.shape, dtype=dtype, device=device))


def _stratified(t: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    cuts = (t[:, 1:] + t[:, :-1]) * 0.5
    lower, upper = torch.cat((t[:, :1], cuts), dim=1), torch.cat((cuts, t[:, -1:]), dim=1)
    return torch.lerp(lower, upper, u)


def generate_samples_from_pdf(bins: torch.Tensor, values: torch.Tensor, n_samples: int, randomize_samples: bool) -> torch.Tensor:
    """Depths of the fine pass (utils.py:78-109): inverse-transform sampling of the piecewise-constant density whose K-2 inner masses
    (`values` without its ends, + 1e-5) sit between the K-1 mid points of `bins`; u is uniform (random or evenly spaced)."""
    rows = bins.shape[0]
    if randomize_samples:
        u = torch.rand(rows, n_samples, device=bins.device)
    else:
        u = torch.linspace(0.0, 1.0, steps=n_samples, device=bins.device).expand(rows, n_samples).contiguous()
    return _samples_from_pdf(bins, values, u)


def _samples_from_pdf(bins: torch.Tensor, values: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    knots = (bins[:, 1:] + bins[:, :-1]) * 0.5
    mass = values[:, 1:-1] + 1e-5
    cdf = torch.nn.functional.pad(torch.cumsum(mass / mass.sum(dim=1, keepdim=True), dim=1), (1, 0))  # cdf[:, 0] = 0
    right = torch.searchsorted(cdf, u, right=True)
    left, right = (right - 1).clamp(min=0), right.clamp(max=cdf.shape[1] - 1)
    c0, c1, k0, k1 = cdf.gather(1, left), cdf.gather(1, right), knots.gather(1, left), knots.gather(1, right)
    width = c1 - c0
    width = torch.where(width < 1e-5, torch.ones_like(width), width)  # empty interval: take its left knot
    return (k0 + (u - c0) / width * (k1 - k0)).detach()


def integrate_samples(depth_samples, ray_directions, densities, colors, background_color, final_delta: float = 1.0e10):
    """Emission-absorption quadrature along each ray (utils.py:112-136).  Segment i spans depth i .. i+1 (the last one `final_delta`), scaled
    by |direction| because depths are in units of the unnormalised ray; opacity_i = 1 - exp(-sigma_i len_i); a sample is weighted by its
    opacity times the transmittance of everything in front.  -> rgb (+ leftover transmittance * background), depth (weighted mean, 0 for
    rays that hit nothing), alpha, weights."""
    pad = torch.nn.functional.pad
    length = pad(torch.diff(depth_samples, dim=-1), (0, 1), value=final_delta) * torch.linalg.vector_norm(ray_directions, dim=-1, keepdim=True)
    opacity = 1.0 - torch.exp(-densities * length)
    through = torch.cumprod(pad(1.0 - opacity, (1, 0), value=1.0), dim=-1)      # through[:, i] = transmittance in front of sample i; [:, -1] = leftover
    weights = opacity * through[:, :-1]
    leftover = through[:, -1:]
    alpha = 1.0 - leftover
    weighted_depth = (weights * depth_samples).sum(dim=-1, keepdim=True)
    depth = torch.where(leftover < 1.0, weighted_depth / alpha, torch.zeros_like(alpha))
    rgb = (weights.unsqueeze(-1) * colors).sum(dim=-2)
    if background_color is not None:
        rgb = rgb + leftover * background_color
    return rgb, depth, alpha, weights


def _rays_eligible(n_coarse: int, n_fine: int, *tensors, grad_ok=()) -> bool:
    """The device path of group 19 takes these tensors: all on one GPU, f32, none requiring grad while autograd records (but for those in `grad_ok`, which
    the caller differentiates itself: group 20), a supported sample count."""
    first = tensors[0]
    if not all(t.is_cuda and t.device == first.device and t.dtype == torch.float32 for t in tensors):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad and not any(t is g for g in grad_ok) for t in tensors):
        return False
    from . import _lib
    return first.shape[0] > 0 and bool(_lib.load().nrc_nerf_rays_supported(int(n_coarse), int(n_fine)))


class _RayPositions(torch.autograd.Function):
    """positions = o + d t behind a sampling kernel that has already produced them (header group 20): the backward is nrc_nerf_positions_backward.  t is a
    constant here (the reference detaches the fine depths; the coarse ones do not depend on the ray)."""

    @staticmethod
    def forward(ctx, origins, directions, t, positions):
        ctx.save_for_backward(t)
        ctx.set_materialize_grads(False)
        return positions.view_as(positions)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_positions):
        if d_positions is None:
            return None, None, None, None
        from . import _lib
        (t,) = ctx.saved_tensors
        n, s = t.shape
        d_positions = d_positions.contiguous().float()
        with torch.cuda.device(t.device):
            d_origins = torch.empty(n, 3, dtype=torch.float32, device=t.device)
            d_directions = torch.empty(n, 3, dtype=torch.float32, device=t.device)
            _lib.check(_lib.load().nrc_nerf_positions_backward(_lib.ptr(d_positions), _lib.ptr(t), n, s, _lib.ptr(d_origins), _lib.ptr(d_directions),
                                                               _lib.stream_of(t)), 'nerf_positions_backward')
        return (d_origins if ctx.needs_input_grad[0] else None, d_directions if ctx.needs_input_grad[1] else None, None, None)


def _attach_rays(origins, directions, t, positions, input_grad):
    """the sampled positions, differentiable with respect to the rays when the caller asked for it and one of them requires grad"""
    if input_grad and torch.is_grad_enabled() and (origins.requires_grad or directions.requires_grad):
        return _RayPositions.apply(origins, directions, t, positions)
    return positions


def sample_coarse(origins: torch.Tensor, directions: torch.Tensor, n_samples: int, near_plane: float, far_plane: float, randomize_samples: bool,
                  u: torch.Tensor | None = None, input_grad: bool = False):
    """Depths of the coarse pass and their positions -> (t (N, S), positions (N S, 3)): `generate_samples` and `o + d t` as one kernel
    (csrc/nerf_rays.hip, header group 19).  With `randomize_samples` the offsets are `u` (N, S), drawn with `torch.rand` exactly as
    `generate_samples` draws them when not given.  Falls back to the torch expressions of `render_rays` -- torch's bits -- for CPU tensors, non-f32
    input, an unsupported S, or origins / directions that require grad.  `input_grad=True`: origins and directions that require grad keep the device
    forward and receive `nrc_nerf_positions_backward`'s outputs (header group 20); t carries no gradient."""
    n = origins.shape[0]
    rays_in = (origins, directions)
    if not _rays_eligible(n_samples, 0, origins, directions, grad_ok=rays_in if input_grad else ()) or (u is not None and not _rays_eligible(n_samples, 0, u)):
        if u is None:
            t = generate_samples(n, n_samples, near_plane, far_plane, randomize_samples, origins.dtype, origins.device)
        else:
            t = _stratified(torch.linspace(near_plane, far_plane, n_samples, dtype=origins.dtype, device=origins.device).expand(n, n_samples), u)
        return t, (origins[:, None, :] + directions[:, None, :] * t[:, :, None]).reshape(-1, 3)
    from . import _lib
    t_row = torch.linspace(near_plane, far_plane, n_samples, dtype=torch.float32, device=origins.device)
    if randomize_samples and u is None:
        u = torch.rand((n, n_samples), dtype=torch.float32, device=origins.device)
    origins, directions, u = origins.detach().contiguous(), directions.detach().contiguous(), None if u is None else u.detach().contiguous()
    with torch.cuda.device(origins.device):
        t = torch.empty(n, n_samples, dtype=torch.float32, device=origins.device)
        positions = torch.empty(n * n_samples, 3, dtype=torch.float32, device=origins.device)
        _lib.check(_lib.load().nrc_nerf_sample_coarse(_lib.ptr(origins), _lib.ptr(directions), _lib.ptr(t_row), _lib.ptr(u), n, int(n_samples), _lib.ptr(t),
                                                      _lib.ptr(positions), _lib.stream_of(origins)), 'nerf_sample_coarse')
    return t, _attach_rays(*rays_in, t, positions, input_grad)


def sample_fine(t_coarse: torch.Tensor, weights: torch.Tensor, n_samples: int, randomize_samples: bool, origins: torch.Tensor, directions: torch.Tensor,
                u: torch.Tensor | None = None, input_grad: bool = False):
    """Depths of the fine pass merged with the coarse ones, and their positions -> (t (N, Sc + Sf) ascending, positions (N (Sc + Sf), 3)):
    `generate_samples_from_pdf`, `sort(cat(t_coarse, t_fine))` and `o + d t` as one kernel (header group 19).  `u`: (N, Sf) per-ray draws or (Sf,) one row
    for all rays; when not given it is drawn (`torch.rand`) or laid out (`torch.linspace(0, 1, Sf)`) exactly as `generate_samples_from_pdf` does.  The
    weights carry no gradient (the reference detaches the fine depths).  Finite inputs are required.  Falls back to the torch expressions of `render_rays`
    for CPU tensors, non-f32 input, unsupported sample counts, or depths / origins / directions that require grad.  `input_grad=True`: origins and
    directions that require grad keep the device forward and receive `nrc_nerf_positions_backward`'s outputs (header group 20); t carries no gradient, and
    depths that require grad still fall back."""
    n, n_coarse = t_coarse.shape
    weights = weights.detach()
    rays_in = (origins, directions)
    if (not _rays_eligible(n_coarse, n_samples, t_coarse, weights, origins, directions, grad_ok=rays_in if input_grad else ())
            or (u is not None and not _rays_eligible(n_coarse, n_samples, u))):
        if u is None:
            t_f = generate_samples_from_pdf(t_coarse, weights, n_samples, randomize_samples)
        else:
            t_f = _samples_from_pdf(t_coarse, weights, u.expand(n, n_samples).contiguous())
        t, _ = torch.sort(torch.cat((t_coarse, t_f), dim=-1), dim=-1)
        return t, (origins[:, None, :] + directions[:, None, :] * t[:, :, None]).reshape(-1, 3)
    from . import _lib
    device = t_coarse.device
    if u is None:
        u = (torch.rand(n, n_samples, device=device) if randomize_samples else torch.linspace(0.0, 1.0, steps=n_samples, device=device))
    if u.shape not in ((n, n_samples), (n_samples,)):
        raise ValueError(f'u has shape {tuple(u.shape)}, expected ({n}, {n_samples}) or ({n_samples},)')
    u = u.detach().contiguous()
    t_coarse, origins, directions = t_coarse.detach().contiguous(), origins.detach().contiguous(), directions.detach().contiguous()
    weights = weights.contiguous()
    total = n_coarse + n_samples
    with torch.cuda.device(device):
        t = torch.empty(n, total, dtype=torch.float32, device=device)
        positions = torch.empty(n * total, 3, dtype=torch.float32, device=device)
        _lib.check(_lib.load().nrc_nerf_sample_fine(_lib.ptr(t_coarse), _lib.ptr(weights), _lib.ptr(u), n_samples if u.dim() == 2 else 0, _lib.ptr(origins),
                                                    _lib.ptr(directions), n, int(n_coarse), int(n_samples), _lib.ptr(t), _lib.ptr(positions), None, None,
                                                    _lib.stream_of(t_coarse)), 'nerf_sample_fine')
    return t, _attach_rays(*rays_in, t, positions, input_grad)


class _Composite(torch.autograd.Function):
    """Compositing forward + backward (header group 19).  Gradients for sigma and rgb; for the directions (through the segment lengths, header group 20)
    when they require grad, which `composite` lets through only with `input_grad=True`; depth is not differentiable."""

    @staticmethod
    def forward(ctx, t, directions, sigma, rgb, background, final_delta):
        from . import _lib
        n, s = t.shape
        with torch.cuda.device(t.device):
            out = torch.empty(n, 3, dtype=torch.float32, device=t.device)
            depth = torch.empty(n, 1, dtype=torch.float32, device=t.device)
            alpha = torch.empty(n, 1, dtype=torch.float32, device=t.device)
            weights = torch.empty(n, s, dtype=torch.float32, device=t.device)
            _lib.check(_lib.load().nrc_nerf_integrate_forward(_lib.ptr(t), _lib.ptr(directions), _lib.ptr(sigma), _lib.ptr(rgb), _lib.ptr(background),
                                                              float(final_delta), n, s, _lib.ptr(out), _lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(weights),
                                                              _lib.stream_of(t)), 'nerf_integrate_forward')
        ctx.final_delta = float(final_delta)
        ctx.save_for_backward(t, directions, sigma, rgb, background)
        ctx.mark_non_differentiable(depth)
        ctx.set_materialize_grads(False)
        return out, depth, alpha, weights

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_rgb, d_depth, d_alpha, d_weights):
        from . import _lib
        t, directions, sigma, rgb, background = ctx.saved_tensors
        n, s = t.shape
        d_rgb, d_alpha, d_weights = (None if g is None else g.contiguous().float() for g in (d_rgb, d_alpha, d_weights))
        with torch.cuda.device(t.device):
            d_sigma = torch.empty_like(sigma)
            d_samples = torch.empty_like(rgb)
            if ctx.needs_input_grad[1]:
                d_directions = torch.empty_like(directions)
                _lib.check(_lib.load().nrc_nerf_integrate_backward_dirs(_lib.ptr(d_rgb), _lib.ptr(d_alpha), _lib.ptr(d_weights), _lib.ptr(t),
                                                                        _lib.ptr(directions), _lib.ptr(sigma), _lib.ptr(rgb), _lib.ptr(background),
                                                                        ctx.final_delta, n, s, _lib.ptr(d_sigma), _lib.ptr(d_samples), _lib.ptr(d_directions),
                                                                        _lib.stream_of(t)), 'nerf_integrate_backward_dirs')
                return None, d_directions, d_sigma, d_samples, None, None
            _lib.check(_lib.load().nrc_nerf_integrate_backward(_lib.ptr(d_rgb), _lib.ptr(d_alpha), _lib.ptr(d_weights), _lib.ptr(t), _lib.ptr(directions),
                                                               _lib.ptr(sigma), _lib.ptr(rgb), _lib.ptr(background), ctx.final_delta, n, s, _lib.ptr(d_sigma),
                                                               _lib.ptr(d_samples), _lib.stream_of(t)), 'nerf_integrate_backward')
        return None, None, d_sigma, d_samples, None, None


def composite(t: torch.Tensor, directions: torch.Tensor, sigma: torch.Tensor, rgb: torch.Tensor, background: torch.Tensor | None,
              final_delta: float = 1.0e10, input_grad: bool = False):
    """`integrate_samples` as one kernel, with a backward kernel behind autograd (csrc/nerf_rays.hip, header group 19) -> rgb (N, 3), depth (N, 1),
    alpha (N, 1), weights (N, S).  t (N, S), directions (N, 3), sigma (N, S), rgb (N, S, 3), background (3,) or None.  sigma and rgb receive gradients
    (first order only); depth is marked non-differentiable, as the reference's own comment on its depth expression asks.  Falls back to
    `integrate_samples` -- torch's bits and torch's autograd -- for CPU tensors, non-f32 input, an unsupported S, or when t, the directions or the
    background require grad.  `input_grad=True`: directions that require grad keep the device path and receive the gradient through the segment lengths
    (t[i+1] - t[i]) |d| (`nrc_nerf_integrate_backward_dirs`, header group 20); a t that requires grad still falls back."""
    tensors = (t, directions, sigma, rgb) + (() if background is None else (background,))
    first = t
    eligible = (t.dim() == 2 and t.shape[0] > 0 and all(x.is_cuda and x.device == first.device and x.dtype == torch.float32 for x in tensors)
                and tuple(sigma.shape) == tuple(t.shape) and tuple(rgb.shape) == (*t.shape, 3) and tuple(directions.shape) == (t.shape[0], 3)
                and (background is None or background.numel() == 3)
                and not (torch.is_grad_enabled() and (t.requires_grad or (directions.requires_grad and not input_grad) or (background is not None and background.requires_grad))))
    if eligible:
        from . import _lib
        eligible = bool(_lib.load().nrc_nerf_rays_supported(int(t.shape[1]), 0))
    if not eligible:
        return integrate_samples(t, directions, sigma, rgb, background, final_delta)
    return _Composite.apply(t.detach().contiguous(), directions.contiguous() if input_grad else directions.detach().contiguous(), sigma.contiguous(), rgb.contiguous(),
                            None if background is None else background.detach().contiguous(), final_delta)


def render_rays(coarse_nerf: NeRFBlock | None, nerf: NeRFBlock, origin, direction, view_direction, near_plane: float, far_plane: float,
                background_color, ray_batch_size: int = 8192, n_samples_coarse_nerf: int = 64, n_samples_nerf: int = 192,
                randomize_samples: bool = False, random_noise_density: float = 0.0, fused: bool = False, fused_train: bool = False,
                device_rays: bool = False, input_grad: bool = False) -> dict[str, torch.Tensor]:
    """NeRFRayRenderingComponent.forward (Renderer.py:29-95): chunked coarse pass -> PDF samples -> sorted union -> fine pass.  `fused`: the two network
    calls go through `fused_forward` (one direction row per ray); with density noise, and wherever `fused_forward` falls back, the torch path runs.
    `fused_train`: they go through `fused_apply` instead -- the training path, differentiable with respect to the blocks' parameters; with density
    noise the torch path runs.  `device_rays`: sampling, compositing and the fine pass's resampling + sort go through `sample_coarse`, `composite` and
    `sample_fine` (one kernel each; the random numbers are drawn in the torch path's shapes and order, so a seed gives the same offsets); composes with
    `fused` / `fused_train` and with the torch block; each of the three falls back to the torch expressions below on its own conditions.
    `input_grad`: handed to `fused_apply`, `sample_coarse`, `sample_fine` and `composite` -- with `fused_train=True, device_rays=True` the whole iteration
    stays on the device while `origin`, `direction` and `view_direction` receive gradients from both passes (header group 20)."""
    def query(block, pos, vd):
        if fused_train and not random_noise_density > 0.0:
            return fused_apply(block, pos.reshape(-1, 3), vd, dir_group=pos.shape[1], input_grad=input_grad)
        if fused and not random_noise_density > 0.0:
            return fused_forward(block, pos.reshape(-1, 3), vd, dir_group=pos.shape[1])
        return block(pos.reshape(-1, 3), vd[:, None, :].expand_as(pos).reshape(-1, 3), random_noise_density)

    use_coarse = coarse_nerf is not None and n_samples_coarse_nerf > 0
    keys = ['rgb', 'alpha', 'depth'] + (['rgb_coarse', 'alpha_coarse', 'depth_coarse'] if use_coarse else [])
    chunks: dict[str, list] = {k: [] for k in keys}
    bg = background_color.to(origin.device)
    for a in range(0, origin.shape[0], ray_batch_size):
        o, d, vd = origin[a:a + ray_batch_size], direction[a:a + ray_batch_size], view_direction[a:a + ray_batch_size]
        n = o.shape[0]
        if device_rays:
            if use_coarse:
                t_c, pos = sample_coarse(o, d, n_samples_coarse_nerf, near_plane, far_plane, randomize_samples, input_grad=input_grad)
                dens, col = query(coarse_nerf, pos.view(n, -1, 3), vd)
                rgb_c, depth_c, alpha_c, w_c = composite(t_c, d, dens.reshape(n, -1), col.reshape(n, -1, 3), bg, input_grad=input_grad)
                t, pos = sample_fine(t_c, w_c, n_samples_nerf, randomize_samples, o, d, input_grad=input_grad)
                chunks['rgb_coarse'].append(rgb_c); chunks['depth_coarse'].append(depth_c); chunks['alpha_coarse'].append(alpha_c)
            else:
                t, pos = sample_coarse(o, d, n_samples_nerf, near_plane, far_plane, randomize_samples, input_grad=input_grad)
            dens, col = query(nerf, pos.view(n, -1, 3), vd)
            rgb, depth, alpha, _ = composite(t, d, dens.reshape(n, -1), col.reshape(n, -1, 3), bg, input_grad=input_grad)
            chunks['rgb'].append(rgb); chunks['depth'].append(depth); chunks['alpha'].append(alpha)
            continue
        if use_coarse:
            t_c = generate_samples(n, n_samples_coarse_nerf, near_plane, far_plane, randomize_samples, o.dtype, o.device)
            pos = o[:, None, :] + d[:, None, :] * t_c[:, :, None]
            dens, col = query(coarse_nerf, pos, vd)
            rgb_c, depth_c, alpha_c, w_c = integrate_samples(t_c, d, dens.reshape(n, -1), col.reshape(n, -1, 3), bg)
            t_f = generate_samples_from_pdf(t_c, w_c, n_samples_nerf, randomize_samples)
            t, _ = torch.sort(torch.cat((t_c, t_f), dim=-1), dim=-1)
            chunks['rgb_coarse'].append(rgb_c); chunks['depth_coarse'].append(depth_c); chunks['alpha_coarse'].append(alpha_c)
        else:
            t = generate_samples(n, n_samples_nerf, near_plane, far_plane, randomize_samples, o.dtype, o.device)
        pos = o[:, None, :] + d[:, None, :] * t[:, :, None]
        dens, col = query(nerf, pos, vd)
        rgb, depth, alpha, _ = integrate_samples(t, d, dens.reshape(n, -1), col.reshape(n, -1, 3), bg)
        chunks['rgb'].append(rgb); chunks['depth'].append(depth); chunks['alpha'].append(alpha)
    return {k: torch.cat(v, dim=0) for k, v in chunks.items()}
