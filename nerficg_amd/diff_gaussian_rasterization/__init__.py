"""nerficg_amd.diff_gaussian_rasterization -- drop-in for the `diff_gaussian_rasterization` package the reference imports
through src/Thirdparty/DiffGaussianRasterization.py:17 (pinned upstream commit 59f5f77e, :9) and drives from
src/Methods/GaussianSplatting/Renderer.py:60-81,94-153,163-183:

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier, viewmatrix, projmatrix,
                                  sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                                        rotations=None, cov3D_precomp=None) -> (color (3,H,W) f32, radii (P,) i32)
    GaussianRasterizer.markVisible(positions) -> bool mask

Gradients flow to every provided input and to `means2D` (the screen-space gradient that densification reads,
src/Methods/GaussianSplatting/Model.py:258).  Backed by libnerficg_hip.so (nrc_gs_*); no CPU fallback.
"""
from __future__ import annotations

import contextlib
import warnings
import weakref
from typing import NamedTuple

import torch

from .. import _lib

__all__ = ['GaussianRasterizationSettings', 'GaussianRasterizer', 'rasterize_gaussians', 'fixed_capacity', 'last_counts', 'last_band_mask', 'check_tile_rows']


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    antialiasing: bool = False   # upstream's trailing field: anti-aliased splats (see GaussianRasterizer.forward)


_CAMERA_BLOCKS: dict = {}
_ADOPTED_BLOCK: list = [None]   # the latest camera block written by nrc_gs_camera_block (gaussian_splatting.make_raster_settings)


def adopt_camera_block(block: torch.Tensor) -> None:
    """Registers a float[38] device block whose slices a GaussianRasterizationSettings is about to carry (viewmatrix = block[:16], projmatrix = block[16:32],
    campos = block[32:35], bg = block[35:38]): _camera_block() then uses it as it is."""
    _ADOPTED_BLOCK[0] = block


def _camera_block(rs, dev) -> torch.Tensor:
    """viewmatrix | projmatrix | campos | bg of the settings as ONE device float[38] (the `camera_dev` block of the C ABI): the camera never
    crosses to the host.  Built with one concatenation when the settings carry tensors this process has not seen yet (same storage, same
    version counter -> same values), so a renderer that draws several passes from one camera pays it once.  During a stream capture it is
    always rebuilt, so that the recorded graph re-reads the (then static) camera tensors on every replay."""
    tensors = (rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg)
    blk = _ADOPTED_BLOCK[0]
    if blk is not None and blk.device == torch.device(dev) and all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
        base = blk.data_ptr()
        if (rs.viewmatrix.data_ptr() == base and rs.projmatrix.data_ptr() == base + 64 and rs.campos.data_ptr() == base + 128 and rs.bg.data_ptr() == base + 140
                and rs.viewmatrix.is_contiguous() and rs.projmatrix.is_contiguous()):
            return blk     # (also inside a stream capture: the launch that fills the block is part of the recording)
    capturing = torch.cuda.is_current_stream_capturing()
    key = tuple((t.data_ptr(), t._version, t.device) for t in tensors)
    hit = None if capturing else _CAMERA_BLOCKS.get(key)
    if hit is None:
        block = torch.cat([t.detach().reshape(-1).to(device=dev, dtype=torch.float32) for t in tensors])
        if block.numel() != 38:
            raise RuntimeError(f'raster settings: viewmatrix (4,4), projmatrix (4,4), campos (3), bg (3) expected, got {block.numel()} values')
        if capturing:
            return block
        if len(_CAMERA_BLOCKS) >= 256:
            _CAMERA_BLOCKS.pop(next(iter(_CAMERA_BLOCKS)))
        hit = _CAMERA_BLOCKS[key] = (block, tensors)  # the tensors are kept alive: their addresses are the key
    return hit[0]


_FIXED_CAPACITY: tuple[int, int] | None = None
_LAST_COUNTS: torch.Tensor | None = None
_FRAME_STATE_SINK: list = [None]   # a list while a GaussianRasterizer.forward is running: the forward appends the frame state that contributions() reads


@contextlib.contextmanager
def fixed_capacity(instances: int, spans: int = 0):
    """Inside the block the rasterizer sizes nothing from device counts: the per-tile lists hold `instances` entries, the binning workspace
    `spans` row-span records (0: the default 4 P + 65536), and the forward reads nothing back -- which is what a HIP-graph capture needs
    (nerficg_amd.graphs.gaussian_splatting_step).  Instances beyond the capacity are dropped; `last_counts()` tells."""
    global _FIXED_CAPACITY
    if instances < 1 or spans < 0:
        raise ValueError('fixed_capacity: instances >= 1, spans >= 0')
    previous, _FIXED_CAPACITY = _FIXED_CAPACITY, (int(instances), int(spans))
    try:
        yield
    finally:
        _FIXED_CAPACITY = previous


def last_counts() -> torch.Tensor | None:
    """DEVICE int64[2] of the most recent forward: (tile, Gaussian) instances and (tile row, Gaussian) spans the frame needed."""
    return _LAST_COUNTS


_LAST_BAND_MASK: torch.Tensor | None = None


def last_band_mask() -> torch.Tensor | None:
    """DEVICE bool (P,) of the most recent forward with `tile_rows`: the Gaussians whose tile rectangle, clipped to the band, is non-empty -- the only
    rows that can carry a non-zero gradient from that band (the `visible` mask of parallel.UnionRowExchange for a band-parallel step).  Written by the
    kernel that makes the rectangles, so it is the binning's own decision.  None after a forward without a band."""
    return _LAST_BAND_MASK


def check_tile_rows(tile_rows, image_height: int) -> tuple[int, int] | None:
    """(begin, n) of a band of 16-pixel tile rows, validated against the frame's gy = ceil(H / 16) rows; None stays None (the whole frame)."""
    if tile_rows is None:
        return None
    begin, n = (int(v) for v in tile_rows)
    gy = (int(image_height) + 15) // 16
    if begin < 0 or n < 1 or begin + n > gy:
        raise ValueError(f'tile_rows = ({begin}, {n}): a band needs begin >= 0, n >= 1 and begin + n <= {gy} tile rows (image height {image_height})')
    return begin, n


_GRAD_RECORDS: dict = {}   # (device, stream) -> (rows, (rows, 16) f32 accumulator records known to be all zero): ONE buffer per device and stream (see backward)
_SPAN_CAPACITY: dict = {}  # (device, P, W, H, band) -> row-span capacity of the binning workspace once the default proved too small
# Speculative sizing of the tile lists (round 4).  The forward used to STOP at the instance count: D2H copy, host wait, allocation, and only then
# the list scatter and the blend -- 33-37 us of idle GPU per frame at 1 M Gaussians (rocprofv3 kernel trace).  Now the lists are sized from the
# counts of the recent frames of the same (device, P, W, H) (largest of the last 16 x 1.3 + 64 K entries), everything is enqueued at once with the
# capacity-checked scatter, and the count travels to pinned host memory on a side stream while the blend kernel runs; the host looks at it
# before returning and repeats the frame with exact sizes in the rare case that it did not fit.  Same lists, same image.
_INSTANCE_HISTORY: dict = {}   # (device, P, W, H, band) -> recent instance counts (band = the tile_rows of the call, None for a whole frame)
_READBACK: dict = {}           # device -> (side stream, pinned int64[2])
SPECULATIVE_SIZING = True
# How the count reaches the host (round 4, later).  The side-stream copy needs an event on the caller's stream between the counting kernels and the list
# scatter -- 6-7 us of idle GPU in the kernel trace -- plus ~20 us of host calls, and the copy itself lands ~15 us after the count exists.  With a
# MAILBOX (include/nerficg_hip.h, nrc_host_mailbox_alloc: pinned, device-mapped, coherent host memory) the last workgroup of the counting kernel
# stores the two counts and this call's ticket straight into host memory and the host polls the ticket: no event, no copy, no second stream.
# A spin that times out (_lib.HostMailbox.TIMEOUT_S) synchronises the stream and looks again; a mailbox still silent then (never observed) is not used again.
COUNT_MAILBOX = True


def _readback(dev):
    hit = _READBACK.get(dev)
    if hit is None:
        hit = _READBACK[dev] = (torch.cuda.Stream(device=dev), torch.empty(2, dtype=torch.int64).pin_memory())
    return hit


def _opt(t):
    """Absent optional inputs arrive as torch.Tensor([]) (1-D, empty), like in the upstream package; a provided tensor of an
    empty scene has more dimensions."""
    return None if t is None or (t.dim() <= 1 and t.numel() == 0) else t


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest=None, raw=False, rest_step=None, tile_rows=None,
                depth_alpha=False, viewmatrix=None, projmatrix=None, campos=None, features=None, absgrad=False, antialiasing=False):
        rs = raster_settings
        lib = _lib.load()
        band = check_tile_rows(tile_rows, rs.image_height)
        depth_alpha = bool(depth_alpha)
        # camera_grad: the three pose tensors of the settings arrive as tensor inputs as well, so that autograd asks this function for their gradients
        ctx.camera = None
        if viewmatrix is not None:     # (rasterize_gaussians has refused rest_step by now)
            needs = tuple(ctx.needs_input_grad[14:17])
            if any(needs):
                ctx.camera = (needs, tuple((tuple(t.shape), t.dtype, t.device) for t in (viewmatrix, projmatrix, campos)))
        if depth_alpha and rest_step is not None:
            raise RuntimeError('return_depth_alpha together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) takes the '
                               'colour gradient only -- there is no depth-and-alpha form of it; render without rest_step and let the optimizer take that step')
        if features is not None and rest_step is not None:
            raise RuntimeError('features together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) takes the '
                               'colour gradient only -- there is no feature form of it; render without rest_step and let the optimizer take that step')
        absgrad = bool(absgrad)
        if absgrad and rest_step is not None:
            raise RuntimeError('absgrad together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) takes the '
                               'colour gradient only -- there is no absgrad form of it; render without rest_step and let the optimizer take that step')
        if absgrad and features is not None:
            raise RuntimeError('absgrad together with features: the feature backward (nrc_gs_backward_features_band) forms its share of dL/dalpha in another kernel, '
                               'and |a + b| per pixel cannot be assembled from two kernels\' sums -- there is no absgrad form of it; render the features in a call of their own')
        antialiasing = bool(antialiasing) or bool(getattr(rs, 'antialiasing', False))
        if antialiasing and rest_step is not None:
            raise RuntimeError(_AA_REST_STEP)
        if antialiasing and viewmatrix is not None:
            raise RuntimeError(_AA_CAMERA_GRAD)
        if band is not None and rest_step is not None:
            raise RuntimeError('rest_step together with tile_rows: the backward pass of a band holds this band\'s SHARE of the gradient only, and an Adam step '
                               'taken on a partial gradient is not the optimizer\'s step -- sum the shares over the bands first and step then')
        dev = means3D.device
        f32 = torch.float32
        prep = lambda t: None if _opt(t) is None else t.detach().to(f32).contiguous()
        means3D_c, sh_c, col_c, op_c = prep(means3D), prep(sh), prep(colors_precomp), prep(opacities)
        sc_c, rot_c, cov_c = prep(scales), prep(rotations), prep(cov3Ds_precomp)
        rest_c = prep(sh_rest)
        raw = bool(raw)
        if not means3D.is_cuda:
            raise RuntimeError('means3D must be a CUDA tensor')
        P = means3D_c.shape[0]
        W, H = int(rs.image_width), int(rs.image_height)
        D = int(rs.sh_degree)
        M = 0 if sh_c is None else int(sh_c.shape[1]) + (0 if rest_c is None else int(rest_c.shape[1]))
        gx, gy = (W + 15) // 16, (H + 15) // 16
        nt = gx * gy
        cam_block = _camera_block(rs, dev)
        i32, u8 = torch.int32, torch.uint8
        n1 = max(P, 1)
        radii = torch.empty(n1, dtype=i32, device=dev)
        depths = torch.empty(n1, dtype=f32, device=dev)
        points_xy = torch.empty(n1, 2, dtype=f32, device=dev)
        conic_opacity = torch.empty(n1, 4, dtype=f32, device=dev)
        rgb = torch.empty(n1, 3, dtype=f32, device=dev)
        clamped = torch.empty(n1, dtype=u8, device=dev)
        cov3D = torch.empty(n1, 6, dtype=f32, device=dev)
        tiles_touched = torch.empty(n1, dtype=i32, device=dev)
        splat = torch.empty(n1, 16, dtype=f32, device=dev)
        tile_counts = torch.empty(nt, dtype=i32, device=dev)
        tile_fill = torch.empty(nt, dtype=i32, device=dev)
        ranges = torch.empty(nt, 2, dtype=i32, device=dev)
        num_rendered = torch.empty(2, dtype=torch.int64, device=dev)
        st = _lib.stream_of(radii)
        fixed = _FIXED_CAPACITY
        if fixed is None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('rasterizer forward: sizing the tile lists reads num_rendered on the host, which a stream capture cannot do -- '
                               'wrap the call in diff_gaussian_rasterization.fixed_capacity(instances, spans)')
        # binning workspace: kept per (device, P, W, H) and regrown when a frame needs more row-span records than it holds (the count comes
        # back with the instance count in the one host read of the forward)
        ws_key = (dev, P, W, H, band)   # a band and a whole frame do not size each other's lists
        span_cap = _SPAN_CAPACITY.get(ws_key, 0) if fixed is None else fixed[1]
        inst_cap = 0 if fixed is None else fixed[0]
        history = _INSTANCE_HISTORY.get(ws_key) if fixed is None else None
        speculative = bool(SPECULATIVE_SIZING and history and P > 0 and gx <= 256 and gy <= 256)   # the span binning path (fixed capacities exist there only)
        if speculative:
            inst_cap = min(int(max(history) * 1.3) + 65536, 0xfffffff0)
        # a band writes its own pixel rows only: the rest of the image is zero, so that the band images of a partition sum (and slice) to the frame
        color = torch.empty(3, H, W, dtype=f32, device=dev) if band is None else torch.zeros(3, H, W, dtype=f32, device=dev)
        # depth and alpha maps (2, H, W): plane 0 = sum w z, plane 1 = sum w; a band writes its own rows only, like the colour
        aux = None if not depth_alpha else (torch.empty(2, H, W, dtype=f32, device=dev) if band is None else torch.zeros(2, H, W, dtype=f32, device=dev))
        band_mask = None if band is None else torch.empty(n1, dtype=u8, device=dev)
        n_contrib = torch.empty(H * W, dtype=i32, device=dev)
        final_T = torch.empty(H * W, dtype=f32, device=dev)
        feat_c = None
        if features is not None:
            feat_c = _check_features(features, P, dev)
        global _LAST_COUNTS

        def preprocess(cap_spans, cap_inst, box=None, ticket=0):
            hist_bytes = int(lib.nrc_gs_bin_hist_bytes(P, W, H, cap_spans))
            hist = torch.empty(hist_bytes // 4, dtype=i32, device=dev) if hist_bytes > 0 else None
            if antialiasing:   # the anti-aliased instance of the per-Gaussian kernel (a whole frame = the band of all gy tile rows)
                b0, bn = band if band is not None else (0, gy)
                _lib.check(lib.nrc_gs_preprocess_antialias_band(
                    P, D, M, W, H, _lib.ptr(means3D_c), _lib.ptr(sh_c), _lib.ptr(rest_c), int(raw), _lib.ptr(col_c), _lib.ptr(op_c), _lib.ptr(sc_c), float(rs.scale_modifier),
                    _lib.ptr(rot_c), _lib.ptr(cov_c), None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(depths),
                    _lib.ptr(points_xy), _lib.ptr(conic_opacity), _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(tiles_touched),
                    _lib.ptr(tile_counts), _lib.ptr(ranges), _lib.ptr(tile_fill), _lib.ptr(hist), cap_spans, cap_inst, _lib.ptr(splat), _lib.ptr(num_rendered),
                    box if hist is not None else None, ticket, b0, bn, _lib.ptr(band_mask), st), 'gs_preprocess_antialias_band')
                return hist
            if band is not None:
                _lib.check(lib.nrc_gs_preprocess_band(
                    P, D, M, W, H, _lib.ptr(means3D_c), _lib.ptr(sh_c), _lib.ptr(rest_c), int(raw), _lib.ptr(col_c), _lib.ptr(op_c), _lib.ptr(sc_c), float(rs.scale_modifier),
                    _lib.ptr(rot_c), _lib.ptr(cov_c), None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(depths),
                    _lib.ptr(points_xy), _lib.ptr(conic_opacity), _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(tiles_touched),
                    _lib.ptr(tile_counts), _lib.ptr(ranges), _lib.ptr(tile_fill), _lib.ptr(hist), cap_spans, cap_inst, _lib.ptr(splat), _lib.ptr(num_rendered),
                    box if hist is not None else None, ticket, band[0], band[1], _lib.ptr(band_mask), st), 'gs_preprocess_band')
                return hist
            _lib.check(lib.nrc_gs_preprocess(
                P, D, M, W, H, _lib.ptr(means3D_c), _lib.ptr(sh_c), _lib.ptr(rest_c), int(raw), _lib.ptr(col_c), _lib.ptr(op_c), _lib.ptr(sc_c), float(rs.scale_modifier),
                _lib.ptr(rot_c), _lib.ptr(cov_c), None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(depths),
                _lib.ptr(points_xy), _lib.ptr(conic_opacity), _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(tiles_touched),
                _lib.ptr(tile_counts), _lib.ptr(ranges), _lib.ptr(tile_fill), _lib.ptr(hist), cap_spans, cap_inst, _lib.ptr(splat), _lib.ptr(num_rendered),
                box if hist is not None else None, ticket, st), 'gs_preprocess')
            return hist

        def bin_render(hist, cap_spans, cap_inst, n_list):
            keys_ = torch.empty(max(n_list, 1) if hist is None else 1, dtype=torch.int64, device=dev)  # only the per-tile key sort fallback uses them
            plist = torch.empty(max(n_list, 1), dtype=i32, device=dev)
            if aux is not None:   # the blend instance that also accumulates depth (a whole frame = the band of all gy tile rows)
                b0, bn = band if band is not None else (0, gy)
                _lib.check(lib.nrc_gs_bin_render_aux_band(P, W, H, None, _lib.ptr(cam_block), _lib.ptr(radii), _lib.ptr(depths), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                                                          _lib.ptr(rgb), _lib.ptr(ranges), _lib.ptr(tile_fill), _lib.ptr(hist), cap_spans, cap_inst, _lib.ptr(keys_), _lib.ptr(plist),
                                                          _lib.ptr(splat), _lib.ptr(color), _lib.ptr(n_contrib), _lib.ptr(final_T), b0, bn, _lib.ptr(aux), st),
                           'gs_bin_render_aux_band')
                return keys_, plist
            if band is not None:
                _lib.check(lib.nrc_gs_bin_render_band(P, W, H, None, _lib.ptr(cam_block), _lib.ptr(radii), _lib.ptr(depths), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                                                      _lib.ptr(rgb), _lib.ptr(ranges), _lib.ptr(tile_fill), _lib.ptr(hist), cap_spans, cap_inst, _lib.ptr(keys_), _lib.ptr(plist),
                                                      _lib.ptr(splat), _lib.ptr(color), _lib.ptr(n_contrib), _lib.ptr(final_T), band[0], band[1], st), 'gs_bin_render_band')
                return keys_, plist
            _lib.check(lib.nrc_gs_bin_render(P, W, H, None, _lib.ptr(cam_block), _lib.ptr(radii), _lib.ptr(depths), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                                             _lib.ptr(rgb), _lib.ptr(ranges), _lib.ptr(tile_fill), _lib.ptr(hist), cap_spans, cap_inst, _lib.ptr(keys_), _lib.ptr(plist),
                                             _lib.ptr(splat), _lib.ptr(color), _lib.ptr(n_contrib), _lib.ptr(final_T), st), 'gs_bin_render')
            return keys_, plist

        done = False
        if speculative:
            mb = _lib.HostMailbox.for_device(dev) if COUNT_MAILBOX else None
            if mb is not None:
                mb.lock.acquire()
            try:
                ticket = mb.next_ticket() if mb is not None else 0
                bin_hist = preprocess(span_cap, inst_cap, mb.ptr if mb is not None else None, ticket)
                have = span_cap if span_cap > 0 else 4 * max(P, 1) + 65536
                counts = None
                if bin_hist is not None and mb is not None:
                    keys, point_list = bin_render(bin_hist, span_cap, inst_cap, inst_cap)
                    counts = mb.counts(ticket, dev)
            finally:
                if mb is not None:
                    mb.lock.release()
            if bin_hist is not None and mb is not None:
                if counts is None:   # (the mailbox retired itself: silent even behind a stream synchronisation)
                    warnings.warn('diff_gaussian_rasterization: the count mailbox did not answer; using the device counters from now on')
                    counts = num_rendered.tolist()
                n_inst, n_spans = counts
                done = n_inst <= inst_cap and n_spans <= have
                if done:
                    point_list = point_list[:max(n_inst, 1)]
                elif n_spans > have:
                    span_cap = _SPAN_CAPACITY[ws_key] = int(n_spans * 1.25) + 65536
            elif bin_hist is not None:
                side, pinned = _readback(dev)
                main = torch.cuda.current_stream(dev)
                counted = torch.cuda.Event()
                counted.record(main)
                with torch.cuda.stream(side):
                    side.wait_event(counted)
                    pinned.copy_(num_rendered, non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(side)
                num_rendered.record_stream(side)
                keys, point_list = bin_render(bin_hist, span_cap, inst_cap, inst_cap)
                copied.synchronize()
                n_inst, n_spans = pinned.tolist()
                done = n_inst <= inst_cap and n_spans <= have
                if done:
                    point_list = point_list[:max(n_inst, 1)]
                elif n_spans > have:
                    span_cap = _SPAN_CAPACITY[ws_key] = int(n_spans * 1.25) + 65536
        if not done:
            inst_cap = 0 if fixed is None else fixed[0]
            while True:
                bin_hist = preprocess(span_cap, inst_cap)
                if fixed is not None:
                    n_inst = inst_cap
                    break
                n_inst, n_spans = num_rendered.tolist()
                have = span_cap if span_cap > 0 else 4 * max(P, 1) + 65536
                if bin_hist is None or n_spans <= have:
                    break
                span_cap = _SPAN_CAPACITY[ws_key] = int(n_spans * 1.25) + 65536
                if len(_SPAN_CAPACITY) > 64:
                    _SPAN_CAPACITY.pop(next(iter(_SPAN_CAPACITY)))
            keys, point_list = bin_render(bin_hist, span_cap, inst_cap, n_inst)
        if fixed is None and P > 0:
            recent = _INSTANCE_HISTORY.setdefault(ws_key, [])
            recent.append(int(n_inst))
            del recent[:-16]
            if len(_INSTANCE_HISTORY) > 64:
                _INSTANCE_HISTORY.pop(next(iter(_INSTANCE_HISTORY)))
        _LAST_COUNTS = num_rendered
        global _LAST_BAND_MASK
        # (the per-tile key sort fallback, which takes the band (0, gy) only, does not write the mask: every visible Gaussian is in that band)
        _LAST_BAND_MASK = None if band is None else ((band_mask[:P] != 0) if bin_hist is not None and P > 0 else (radii[:P] > 0))
        feature_map = None
        if feat_c is not None:
            # the feature pass: one launch on the state the colour pass just left (lists, tile order, records, n_contrib); a band writes its own rows only
            C_f = int(feat_c.shape[1])
            feature_map = torch.empty(C_f, H, W, dtype=f32, device=dev) if band is None else torch.zeros(C_f, H, W, dtype=f32, device=dev)
            b0, bn = band if band is not None else (0, gy)
            _lib.check(lib.nrc_gs_render_features_band(P, C_f, W, H, _lib.ptr(feat_c), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_fill),
                                                       _lib.ptr(n_contrib), b0, bn, _lib.ptr(feature_map), st), 'gs_render_features_band')
        if _FRAME_STATE_SINK[0] is not None:   # GaussianRasterizer.forward is the caller: what contributions() runs on (references only, nothing is created for it)
            _FRAME_STATE_SINK[0].append(dict(point_list=point_list, ranges=ranges, splat=splat, tile_fill=tile_fill, n_contrib=n_contrib, dims=(P, W, H), band=band))
        ctx.features = feat_c
        ctx.features_grad = feat_c is not None and bool(ctx.needs_input_grad[17])
        ctx.band = band
        ctx.depth_alpha = depth_alpha
        # absgrad: the backward leaves sum_pixels |dL_pixel/dmean2D| on the tensor OBJECT the caller passed as means2D (weakly held: ctx must not keep it alive)
        ctx.absgrad = weakref.ref(means2D) if absgrad else None
        ctx.antialiasing = antialiasing
        ctx.raster_settings = rs
        ctx.dims = (P, D, M, W, H)
        ctx.num_rendered = n_inst if fixed is None else -1
        ctx.has = (sh_c is not None, col_c is not None, sc_c is not None, cov_c is not None)
        ctx.opacity_shape = tuple(opacities.shape)
        ctx.save_for_backward(means3D_c, sh_c if sh_c is not None else torch.empty(0), col_c if col_c is not None else torch.empty(0),
                              sc_c if sc_c is not None else torch.empty(0), rot_c if rot_c is not None else torch.empty(0),
                              cov_c if cov_c is not None else torch.empty(0), radii, points_xy, conic_opacity, rgb, clamped, cov3D,
                              point_list, ranges, n_contrib, final_T, splat, tile_fill, rest_c if rest_c is not None else torch.empty(0), op_c, cam_block)
        ctx.raw, ctx.has_rest = raw, rest_c is not None
        ctx.rest_step = rest_step
        if rest_step is not None and (rest_c is None or rest_c.data_ptr() != sh_rest.data_ptr() or sc_c is None or col_c is not None or cov_c is not None):
            raise RuntimeError('rest_step: needs shs_rest as a contiguous f32 CUDA tensor (updated in place), scales / rotations, no colors_precomp / cov3D_precomp')
        ctx.debug_state = dict(depths=depths, tiles_touched=tiles_touched, keys=keys, point_list=point_list, ranges=ranges, n_contrib=n_contrib, final_T=final_T,
                               num_rendered=num_rendered)
        radii_out = radii[:P]
        ctx.mark_non_differentiable(radii_out)
        # radii carry no gradient: without this autograd hands the backward a zero-filled (P,) int tensor for them -- a 4 MB fill launch per step
        ctx.set_materialize_grads(False)
        if depth_alpha:
            return (color, radii_out, aux[0], aux[1]) + (() if feature_map is None else (feature_map,))
        return (color, radii_out) + (() if feature_map is None else (feature_map,))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out_color, _grad_radii, *grad_extra):   # the extra output gradients: depth and alpha (a forward with depth_alpha), then the feature map
        grad_depth_alpha = grad_extra[:2] if ctx.depth_alpha else ()
        grad_feature_map = grad_extra[2 if ctx.depth_alpha else 0] if ctx.features is not None else None
        (means3D, sh, col, sc, rot, cov, radii, points_xy, conic_opacity, rgb, clamped, cov3D, point_list, ranges, n_contrib,
         final_T, splat, tile_order, sh_rest, opac, cam_block) = ctx.saved_tensors
        raw, has_rest = ctx.raw, ctx.has_rest
        has_sh, has_col, has_sr, has_cov = ctx.has
        P, D, M, W, H = ctx.dims
        rs = ctx.raster_settings
        lib = _lib.load()
        dev = means3D.device
        f32 = torch.float32
        if grad_out_color is None:   # (grads are not materialised: the image did not take part in the loss)
            grad_out_color = torch.zeros(3, H, W, dtype=f32, device=dev)
        g = grad_out_color.to(f32).contiguous()
        g_aux = None
        if ctx.depth_alpha:   # (2, H, W): dL/ddepth, dL/dalpha; a map that did not take part in the loss counts as zero
            g_aux = torch.zeros(2, H, W, dtype=f32, device=dev)
            for k, gk in enumerate(grad_depth_alpha[:2]):
                if gk is not None:
                    g_aux[k].copy_(gk.reshape(H, W))
        n1 = max(P, 1)
        dmean2D = torch.empty(n1, 3, dtype=f32, device=dev)
        # workspace: one 64-byte accumulator record per Gaussian.  The per-Gaussian backward clears every record it reads, so the buffer of the
        # previous backward of the same size is all zero again and is reused without a clearing launch (one buffer per device, size and stream).
        # A recording (HIP-graph capture) takes a buffer of its own and keeps the clearing launch: the recorded pointer must not be shared.
        capturing = torch.cuda.is_current_stream_capturing()
        rec_key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        kept = None if capturing else _GRAD_RECORDS.pop(rec_key, None)
        # the kept buffer serves the same number of Gaussians only (densification changes P every few hundred steps: the old buffer is dropped then,
        # not parked -- eight parked sizes were ~3 GB at 6 M Gaussians, advisor finding of round 4)
        grad_records = kept[1] if kept is not None and kept[0] == n1 else None
        records_clear = grad_records is not None
        if grad_records is None:
            grad_records = torch.empty(n1, 16, dtype=f32, device=dev)
        dcolor = torch.empty(n1, 3, dtype=f32, device=dev) if has_col else None   # only a caller with colors_precomp asks for it
        dopacity = torch.empty(n1, dtype=f32, device=dev)
        dmean3D = torch.empty(n1, 3, dtype=f32, device=dev)
        dcov3D = torch.empty(n1, 6, dtype=f32, device=dev)
        dsh = torch.empty(n1, 1 if has_rest else max(M, 1), 3, dtype=f32, device=dev) if has_sh else None
        rest_step = ctx.rest_step
        dsh_rest = torch.empty(n1, M - 1, 3, dtype=f32, device=dev) if has_rest and rest_step is None else None
        dscale = torch.empty(n1, 3, dtype=f32, device=dev) if has_sr else None
        drot = torch.empty(n1, 4, dtype=f32, device=dev) if has_sr else None
        dfeat = None
        feat = ctx.features
        if feat is not None:
            # The feature backward goes FIRST: it leaves its geometry sums in slots [3..8] of the records, the colour backward below adds its own and its
            # per-Gaussian part consumes and clears both.  A missing output gradient counts as zero: no launch, exact zeros for `features`.
            C_f = int(feat.shape[1])
            if grad_feature_map is not None and P > 0:
                g_f = grad_feature_map.to(f32).reshape(C_f, H, W).contiguous()
                dfeat = torch.empty(n1, C_f, dtype=f32, device=dev) if ctx.features_grad else None
                b0, bn = ctx.band if ctx.band is not None else (0, (H + 15) // 16)
                _lib.check(lib.nrc_gs_backward_features_band(P, C_f, W, H, _lib.ptr(feat), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order),
                                                             _lib.ptr(n_contrib), _lib.ptr(final_T), _lib.ptr(g_f), _lib.ptr(dfeat), _lib.ptr(grad_records),
                                                             int(records_clear), b0, bn, _lib.stream_of(g)), 'gs_backward_features_band')
                records_clear = True
            elif ctx.features_grad:
                dfeat = torch.zeros(n1, C_f, dtype=f32, device=dev)
        dcam = None
        if ctx.antialiasing:
            # the anti-aliased instance of the per-Gaussian backward behind the same blend backward; the maps' gradients and the absgrad sums stay optional.  The
            # activated opacities the forward read are handed over also without raw parameters: dL/dcov2D through comp carries them
            b0, bn = ctx.band if ctx.band is not None else (0, (H + 15) // 16)
            dabs = torch.empty(P, 3, dtype=f32, device=dev) if ctx.absgrad is not None else None
            _lib.check(lib.nrc_gs_backward_antialias_band(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh if has_sh else None), _lib.ptr(sh_rest if has_rest else None), int(raw),
                _lib.ptr(opac), _lib.ptr(col if has_col else None),
                _lib.ptr(sc if has_sr else None), float(rs.scale_modifier), _lib.ptr(rot if has_sr else None), _lib.ptr(cov if has_cov else None),
                None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), None, _lib.ptr(dopacity), _lib.ptr(dcolor), _lib.ptr(dmean3D), _lib.ptr(dcov3D),
                _lib.ptr(dsh), _lib.ptr(dsh_rest), _lib.ptr(dscale), _lib.ptr(drot), _lib.ptr(grad_records), int(records_clear), b0, bn, _lib.ptr(g_aux),
                None, None, _lib.ptr(dabs) if dabs is not None and P > 0 else None, _lib.stream_of(g)), 'gs_backward_antialias_band')
            if dabs is not None:
                _leave_absgrad(ctx.absgrad(), dabs)
        elif ctx.absgrad is not None:
            # the instances of the blend backward that also sum |dL_pixel/dmean2D| (slots [10], [11] of the records), with or without the maps and the camera gradient
            b0, bn = ctx.band if ctx.band is not None else (0, (H + 15) // 16)
            partials = None
            if ctx.camera is not None:
                partials = torch.empty(int(lib.nrc_gs_pose_partials_floats(P)), dtype=f32, device=dev)
                dcam = torch.empty(35, dtype=f32, device=dev)
            dabs = torch.empty(P, 3, dtype=f32, device=dev)   # (every row is written; P == 0: nothing to write)
            _lib.check(lib.nrc_gs_backward_absgrad_band(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh if has_sh else None), _lib.ptr(sh_rest if has_rest else None), int(raw),
                _lib.ptr(opac if raw else None), _lib.ptr(col if has_col else None),
                _lib.ptr(sc if has_sr else None), float(rs.scale_modifier), _lib.ptr(rot if has_sr else None), _lib.ptr(cov if has_cov else None),
                None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), None, _lib.ptr(dopacity), _lib.ptr(dcolor), _lib.ptr(dmean3D), _lib.ptr(dcov3D),
                _lib.ptr(dsh), _lib.ptr(dsh_rest), _lib.ptr(dscale), _lib.ptr(drot), _lib.ptr(grad_records), int(records_clear), b0, bn, _lib.ptr(g_aux),
                _lib.ptr(partials), _lib.ptr(dcam), _lib.ptr(dabs) if P > 0 else None, _lib.stream_of(g)), 'gs_backward_absgrad_band')
            _leave_absgrad(ctx.absgrad(), dabs)
        elif ctx.camera is not None:
            # the same backward with two extra launches between the blend backward and the per-Gaussian backward: dL/d(viewmatrix | projmatrix | campos) as float[35]
            b0, bn = ctx.band if ctx.band is not None else (0, (H + 15) // 16)
            partials = torch.empty(int(lib.nrc_gs_pose_partials_floats(P)), dtype=f32, device=dev)
            dcam = torch.empty(35, dtype=f32, device=dev)
            _lib.check(lib.nrc_gs_backward_pose_band(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh if has_sh else None), _lib.ptr(sh_rest if has_rest else None), int(raw),
                _lib.ptr(opac if raw else None), _lib.ptr(col if has_col else None),
                _lib.ptr(sc if has_sr else None), float(rs.scale_modifier), _lib.ptr(rot if has_sr else None), _lib.ptr(cov if has_cov else None),
                None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), None, _lib.ptr(dopacity), _lib.ptr(dcolor), _lib.ptr(dmean3D), _lib.ptr(dcov3D),
                _lib.ptr(dsh), _lib.ptr(dsh_rest), _lib.ptr(dscale), _lib.ptr(drot), _lib.ptr(grad_records), int(records_clear), b0, bn, _lib.ptr(g_aux),
                _lib.ptr(partials), _lib.ptr(dcam), _lib.stream_of(g)), 'gs_backward_pose_band')
        elif rest_step is not None:
            # the optimizer step of the `rest` SH tensor inside the preprocessing backward (nrc_gs_backward_rest_step): no gradient tensor for it
            param, m_rest, v_rest, lr, beta1, beta2, eps, bc1, bc2 = rest_step.take()
            if param.data_ptr() != sh_rest.data_ptr():
                raise RuntimeError('rest_step: the tensor to update is not the one the forward pass read')
            _lib.check(lib.nrc_gs_backward_rest_step(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh), _lib.ptr(sh_rest), int(raw), _lib.ptr(opac if raw else None), _lib.ptr(sc), float(rs.scale_modifier),
                _lib.ptr(rot), _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity), _lib.ptr(rgb),
                _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), _lib.ptr(dopacity), _lib.ptr(dmean3D), _lib.ptr(dcov3D), _lib.ptr(dsh), _lib.ptr(dscale), _lib.ptr(drot),
                _lib.ptr(grad_records), int(records_clear), _lib.ptr(m_rest), _lib.ptr(v_rest), float(lr), float(beta1), float(beta2), float(eps), float(bc1), float(bc2),
                _lib.stream_of(g)), 'gs_backward_rest_step')
            torch.autograd.graph.increment_version(param)      # written through a raw pointer
        elif g_aux is not None:
            b0, bn = ctx.band if ctx.band is not None else (0, (H + 15) // 16)
            _lib.check(lib.nrc_gs_backward_aux_band(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh if has_sh else None), _lib.ptr(sh_rest if has_rest else None), int(raw),
                _lib.ptr(opac if raw else None), _lib.ptr(col if has_col else None),
                _lib.ptr(sc if has_sr else None), float(rs.scale_modifier), _lib.ptr(rot if has_sr else None), _lib.ptr(cov if has_cov else None),
                None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), None, _lib.ptr(dopacity), _lib.ptr(dcolor), _lib.ptr(dmean3D), _lib.ptr(dcov3D),
                _lib.ptr(dsh), _lib.ptr(dsh_rest), _lib.ptr(dscale), _lib.ptr(drot), _lib.ptr(grad_records), int(records_clear), b0, bn, _lib.ptr(g_aux),
                _lib.stream_of(g)), 'gs_backward_aux_band')
        elif ctx.band is not None:
            # this band's share of every gradient: the blend backward over the band's tiles, the per-Gaussian backward over all P
            _lib.check(lib.nrc_gs_backward_band(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh if has_sh else None), _lib.ptr(sh_rest if has_rest else None), int(raw),
                _lib.ptr(opac if raw else None), _lib.ptr(col if has_col else None),
                _lib.ptr(sc if has_sr else None), float(rs.scale_modifier), _lib.ptr(rot if has_sr else None), _lib.ptr(cov if has_cov else None),
                None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), None, _lib.ptr(dopacity), _lib.ptr(dcolor), _lib.ptr(dmean3D), _lib.ptr(dcov3D),
                _lib.ptr(dsh), _lib.ptr(dsh_rest), _lib.ptr(dscale), _lib.ptr(drot), _lib.ptr(grad_records), int(records_clear), ctx.band[0], ctx.band[1],
                _lib.stream_of(g)), 'gs_backward_band')
        else:
            _lib.check(lib.nrc_gs_backward(
                P, D, M, W, H, None, _lib.ptr(means3D), _lib.ptr(sh if has_sh else None), _lib.ptr(sh_rest if has_rest else None), int(raw),
                _lib.ptr(opac if raw else None), _lib.ptr(col if has_col else None),
                _lib.ptr(sc if has_sr else None), float(rs.scale_modifier), _lib.ptr(rot if has_sr else None), _lib.ptr(cov if has_cov else None),
                None, None, None, _lib.ptr(cam_block), float(rs.tanfovx), float(rs.tanfovy), _lib.ptr(radii), _lib.ptr(points_xy), _lib.ptr(conic_opacity),
                _lib.ptr(rgb), _lib.ptr(clamped), _lib.ptr(cov3D), _lib.ptr(point_list), _lib.ptr(ranges), _lib.ptr(splat), _lib.ptr(tile_order), _lib.ptr(n_contrib), _lib.ptr(final_T),
                _lib.ptr(g), _lib.ptr(dmean2D), None, _lib.ptr(dopacity), _lib.ptr(dcolor), _lib.ptr(dmean3D), _lib.ptr(dcov3D),
                _lib.ptr(dsh), _lib.ptr(dsh_rest), _lib.ptr(dscale), _lib.ptr(drot), _lib.ptr(grad_records), int(records_clear), _lib.stream_of(g)), 'gs_backward')
        if not capturing and P > 0:   # (P == 0: the library returned before touching the uninitialised buffer -- it is NOT known to be zero)
            _GRAD_RECORDS[rec_key] = (n1, grad_records)   # only after a call that went through: a failed one leaves the entry popped (contents unknown)
        cut = (lambda t: t) if P == n1 else (lambda t: t[:P])     # (whole buffers when nothing is cut: a gradient that is not a view can be adopted as .grad without a copy)
        grads = (cut(dmean3D), cut(dmean2D), cut(dsh) if has_sh else None, cut(dcolor) if has_col else None,
                 cut(dopacity).reshape(ctx.opacity_shape), cut(dscale) if has_sr else None, cut(drot) if has_sr else None,
                 cut(dcov3D) if has_cov else None, None, cut(dsh_rest) if dsh_rest is not None else None, None, None, None, None) + _camera_grads(ctx.camera, dcam, feat is not None) \
            + (() if feat is None else (cut(dfeat) if dfeat is not None else None,))
        if ctx.absgrad is not None:   # the call passed every input up to the flag: their positions are filled
            grads += (None,) * (19 - len(grads))
        if ctx.antialiasing:          # (likewise: 20 inputs)
            grads += (None,) * (20 - len(grads))
        return grads


_AA_REST_STEP = ('antialiasing together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) has no anti-aliased form -- '
                 'its per-Gaussian kernel does not carry the gradient through the opacity compensation; render without rest_step and let the optimizer take that step')
_AA_CAMERA_GRAD = ('antialiasing together with camera_grad: the camera backward (nrc_gs_backward_pose_band) has no anti-aliased form -- the opacity compensation '
                   'depends on the pose through the projected covariance, and that path is not built; render without camera_grad, or without antialiasing')


def _leave_absgrad(target, dabs) -> None:
    """`means2D.absgrad` of a backward with absgrad=True.  Like .grad it accumulates: two bands rendered on one leaf sum to the frame."""
    if target is None:
        return
    have = getattr(target, 'absgrad', None)
    if torch.is_tensor(have) and have.shape == dabs.shape and have.dtype == torch.float32 and have.device == dabs.device:
        have.add_(dabs)
    else:
        target.absgrad = dabs


def _check_features(features, P: int, dev) -> torch.Tensor:
    """`features` as the (P, C) f32 contiguous tensor the feature pass reads; ValueError / RuntimeError naming the argument otherwise."""
    if not torch.is_tensor(features):
        raise ValueError(f'features must be a (P, C) float32 CUDA tensor, got {type(features).__name__}')
    if not features.is_cuda or features.device != dev:
        raise RuntimeError(f'features must be a CUDA tensor on the device of means3D ({dev}), got {features.device}')
    if features.dtype != torch.float32:
        raise ValueError(f'features must have dtype torch.float32, got {features.dtype}')
    if features.dim() != 2 or features.shape[0] != P:
        raise ValueError(f'features must have shape (P, C) = ({P}, C), got {tuple(features.shape)}')
    if not 1 <= features.shape[1] <= 256:
        raise ValueError(f'features: C = {features.shape[1]} channels, 1 <= C <= 256 are supported')
    return features.detach().contiguous()


def _camera_grads(camera, dcam, placeholders=False):
    """The backward's float[35] as the gradients of viewmatrix, projmatrix and campos, each in its tensor's own shape, dtype and device (None where none is needed).
    `placeholders`: three Nones when the pose tensors were no inputs but a later input (features) needs their positions filled."""
    if camera is None:
        return (None, None, None) if placeholders else ()
    needs, like = camera
    parts = (dcam[:16], dcam[16:32], dcam[32:35])
    return tuple(part.reshape(shape).to(device=device, dtype=dtype) if need else None for need, part, (shape, dtype, device) in zip(needs, parts, like))


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest=None, raw=False, rest_step=None, tile_rows=None,
                        return_depth_alpha=False, camera_grad=False, features=None, absgrad=False, antialiasing=False):
    """`tile_rows` = (begin, n): render and differentiate the band of 16-pixel tile rows [begin, begin + n) only (see GaussianRasterizer.forward); None: the frame.
    `return_depth_alpha`: (image, radii, depth, alpha) instead of (image, radii) -- see GaussianRasterizer.forward.
    `camera_grad`: gradients to raster_settings.viewmatrix / projmatrix / campos, for those that require grad -- see GaussianRasterizer.forward.
    `features`: a (P, C) tensor blended by the colour's weights; appends feature_map (C, H, W) to the outputs -- see GaussianRasterizer.forward.
    `absgrad`: the backward also leaves sum_pixels |dL_pixel/dmean2D| as means2D.absgrad -- see GaussianRasterizer.forward.
    `antialiasing` (or raster_settings.antialiasing): anti-aliased splats, the blended opacity is o * comp -- see GaussianRasterizer.forward."""
    if antialiasing or getattr(raster_settings, 'antialiasing', False):
        if rest_step is not None:
            raise RuntimeError(_AA_REST_STEP)
        if camera_grad:
            raise RuntimeError(_AA_CAMERA_GRAD)
        if absgrad and features is not None:
            raise RuntimeError('absgrad together with features: the feature backward (nrc_gs_backward_features_band) forms its share of dL/dalpha in another kernel, '
                               'and |a + b| per pixel cannot be assembled from two kernels\' sums -- there is no absgrad form of it; render the features in a call of their own')
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, None,
                                         None if tile_rows is None else tuple(int(v) for v in tile_rows), bool(return_depth_alpha), None, None, None, features,
                                         bool(absgrad), True)
    if absgrad:
        if rest_step is not None:
            raise RuntimeError('absgrad together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) takes the '
                               'colour gradient only -- there is no absgrad form of it; render without rest_step and let the optimizer take that step')
        if features is not None:
            raise RuntimeError('absgrad together with features: the feature backward (nrc_gs_backward_features_band) forms its share of dL/dalpha in another kernel, '
                               'and |a + b| per pixel cannot be assembled from two kernels\' sums -- there is no absgrad form of it; render the features in a call of their own')
        rs = raster_settings
        pose = (None, None, None)
        if camera_grad and torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
            pose = (rs.viewmatrix, rs.projmatrix, rs.campos)
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, None,
                                         None if tile_rows is None else tuple(int(v) for v in tile_rows), bool(return_depth_alpha), *pose, None, True)
    if features is not None:
        if rest_step is not None:
            raise RuntimeError('features together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) takes the '
                               'colour gradient only -- there is no feature form of it; render without rest_step and let the optimizer take that step')
        rs = raster_settings
        pose = (None, None, None)
        if camera_grad and torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
            pose = (rs.viewmatrix, rs.projmatrix, rs.campos)
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, None,
                                         None if tile_rows is None else tuple(int(v) for v in tile_rows), bool(return_depth_alpha), *pose, features)
    if camera_grad:
        if rest_step is not None:
            raise RuntimeError('camera_grad together with rest_step: the backward pass that steps the `rest` SH tensor (nrc_gs_backward_rest_step) has no camera '
                               'gradient; render without rest_step and let the optimizer take that step')
        rs = raster_settings
        pose = (rs.viewmatrix, rs.projmatrix, rs.campos)
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in pose):
            return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, None,
                                             None if tile_rows is None else tuple(int(v) for v in tile_rows), bool(return_depth_alpha), *pose)
    if return_depth_alpha:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, rest_step,
                                         None if tile_rows is None else tuple(int(v) for v in tile_rows), True)
    if tile_rows is None:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, rest_step)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest, raw, rest_step,
                                     tuple(int(v) for v in tile_rows))


class GaussianRasterizer(torch.nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings) -> None:
        super().__init__()
        self.raster_settings = raster_settings
        self._frame_state = None   # of this object's most recent forward call: see contributions()

    def release_state(self) -> None:
        """Drops the references to the most recent forward's frame state (tile lists, ranges, splat records, tile order, n_contrib) that contributions() reads."""
        self._frame_state = None

    def contributions(self, pixel_weights=None, *, out=None, weight_sum=True, weight_max=True, hits=True, clear=False):
        """Per-Gaussian contribution statistics of the view THIS OBJECT'S MOST RECENT forward call rendered (C ABI group 22, csrc/gs_contrib.hip): what pruning
        and scoring methods ask of a view -- RadSplat's maximum blending weight, the hit counts and importance sums of LightGaussian / Mini-Splatting,
        error-weighted scores as in Taming-3DGS, or simply which Gaussians no view sees.  That call may have been a training call or one under torch.no_grad(), a whole
        frame or a `tile_rows` band (the band's pixels only: the bands of a partition add up to the frame).  One launch on the state the colour pass left; no
        preprocess, sort or binning; nothing is differentiable and nothing any other call returns changes.
        With the colour pass's own blended set and weights w_i(p) = alpha_i T_i (bit for bit) and m = `pixel_weights`, an (H, W) float32 CUDA tensor of finite
        values (None: 1 everywhere), a pixel PARTICIPATES iff m(p) != 0, and per Gaussian i
            'weight_sum' (P,) float32   += sum over the participating pixels that blended i of m(p) w_i(p)       (f32 sums: two runs agree to rounding)
            'weight_max' (P,) float32    = max(itself, the largest such w_i(p))                                  (exact: the colour's w)
            'hits'       (P,) int32     += the number of such pixels                                             (exact)
        Returns a dict of the requested statistics (`weight_sum`, `weight_max`, `hits` = False leaves one out; not all three).  `out`: a dict an earlier call
        returned, for the same P and device -- the call ACCUMULATES into its tensors (one call per view gives the multi-view statistics) and returns it;
        `clear=True` zeroes the requested ones first.  Gaussians outside every tile list are untouched.  It is a second call, not a forward argument, so that m
        can be computed from the rendered image: render -> m from the image -> contributions(m).
        The forward keeps references to point_list, ranges, the splat records, the tile order and n_contrib on this object (tensors it creates anyway): they
        stay alive until the next forward call of this object or release_state().  RuntimeError naming the problem: no forward call yet, `pixel_weights` of a wrong
        shape, dtype or device, an `out` that does not match."""
        state = self._frame_state
        if state is None:
            raise RuntimeError('contributions: this rasterizer object has not rendered anything yet (or release_state() was called) -- call it after a forward call')
        wanted = [k for k, on in (('weight_sum', weight_sum), ('weight_max', weight_max), ('hits', hits)) if on]
        if not wanted:
            raise RuntimeError('contributions: at least one of weight_sum, weight_max and hits must be requested')
        P, W, H = state['dims']
        dev = state['n_contrib'].device
        dtypes = dict(weight_sum=torch.float32, weight_max=torch.float32, hits=torch.int32)
        m = None
        if pixel_weights is not None:
            if not torch.is_tensor(pixel_weights) or not pixel_weights.is_cuda or pixel_weights.device != dev:
                raise RuntimeError(f'contributions: pixel_weights must be a CUDA tensor on the device of the rendered frame ({dev}), got '
                                   f'{pixel_weights.device if torch.is_tensor(pixel_weights) else type(pixel_weights).__name__}')
            if pixel_weights.dtype != torch.float32:
                raise RuntimeError(f'contributions: pixel_weights must have dtype torch.float32, got {pixel_weights.dtype}')
            if tuple(pixel_weights.shape) != (H, W):
                raise RuntimeError(f'contributions: pixel_weights must have shape (H, W) = ({H}, {W}), got {tuple(pixel_weights.shape)}')
            m = pixel_weights.detach().contiguous()
        fresh = out is None
        if fresh:
            out = {k: torch.empty(P, dtype=dtypes[k], device=dev) for k in wanted}
        else:
            if not isinstance(out, dict):
                raise RuntimeError(f'contributions: out must be a dict an earlier call returned, got {type(out).__name__}')
            for k in wanted:
                t = out.get(k)
                if not torch.is_tensor(t):
                    raise RuntimeError(f'contributions: out has no tensor {k!r} (request the same statistics as the call that made it)')
                if tuple(t.shape) != (P,) or t.dtype != dtypes[k] or t.device != dev or not t.is_contiguous():
                    raise RuntimeError(f'contributions: out[{k!r}] must be a contiguous ({P},) {dtypes[k]} tensor on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}')
        if P > 0:
            band = state['band'] if state['band'] is not None else (0, (H + 15) // 16)
            lib = _lib.load()
            get = lambda k: _lib.ptr(out[k]) if k in wanted else None
            _lib.check(lib.nrc_gs_contributions_band(P, W, H, _lib.ptr(state['point_list']), _lib.ptr(state['ranges']), _lib.ptr(state['splat']), _lib.ptr(state['tile_fill']),
                                                     _lib.ptr(state['n_contrib']), _lib.ptr(m), get('weight_sum'), get('weight_max'), get('hits'), int(fresh or clear),
                                                     band[0], band[1], _lib.stream_of(state['n_contrib'])), 'gs_contributions_band')
        return out

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Frustum test of the upstream rasterizer: view-space z > 0.2."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix.to(positions.device, torch.float32)  # (4,4) = w2c.T
            z = positions.float() @ vm[:3, 2] + vm[3, 2]
            return z > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, shs_rest=None,
                raw_parameters=False, rest_step=None, tile_rows=None, return_depth_alpha=False, camera_grad=False, features=None, absgrad=False, antialiasing=False):
        """The reference's call (Renderer.py:75-81) plus two keyword extensions for callers that own the model tensors: `shs_rest` -- `shs` is then
        (`rest_step`, round 6: an object whose take() returns (parameter, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, bc1, bc2) -- the backward pass then applies
        the optimizer's Adam step to shs_rest itself and returns no gradient for it: nerficg_amd.gaussian_splatting.RestStep)
        the DC part (P,1,3) and shs_rest the (P,M-1,3) remainder, the concatenation of Gaussians.get_features is never built; `raw_parameters` --
        opacities are logits, scales log-scales, rotations unnormalised: the activations of Model.py:45-87 run inside the preprocess kernel and the
        gradients come back w.r.t. the raw tensors.
        `tile_rows` = (begin, n): ONE BAND of the frame, the 16-pixel tile rows [begin, begin + n) of its ceil(H / 16) rows -- the unit a single view is sharded
        by across GPUs (nerficg_amd.parallel.tile_row_band).  The image is still (3, H, W), its band rows bit for bit those of the whole-frame call and zero
        elsewhere (the band images of a partition sum and slice to the frame); `radii` is the full (P,) tensor, identical for every band; the backward pass
        returns this band's SHARE of every gradient, `means2D` included (the shares of a partition sum to the whole-frame gradient, rows of Gaussians that miss
        the band are exactly zero: last_band_mask()).  Not together with `rest_step`.  None (default): the whole frame, today's call.
        `return_depth_alpha=True`: the call returns (image, radii, depth, alpha).  depth and alpha are (H, W) float32 maps blended with the colour's own weights
        w_i = alpha_i T_i and background 0: depth = sum w_i z_i with z_i the view-space depth the sort orders by (ACCUMULATED, not normalised: divide by alpha
        for an expected depth), alpha = sum w_i = 1 - T_final.  Both are differentiable (a map that takes no part in the loss counts as a zero gradient); image,
        radii and everything the backward saves are bit for bit those of the call without the flag.  Works with every parameter form above, with `tile_rows`
        (band rows written, zero elsewhere) and inside fixed_capacity; not together with `rest_step` (RuntimeError).
        `camera_grad=True`: the settings' `viewmatrix`, `projmatrix` and `campos` that require grad receive a gradient, each in its own shape, dtype and device
        (`bg` and the intrinsics receive none).  Everything else the call returns is bit for bit that of the call without the flag, and every other gradient comes from the same
        launches on the same per-Gaussian sums: the backward pass runs two more launches (a reduction over the Gaussians in a fixed order, no atomics) and reads nothing back.  Works with every parameter
        form above, with `tile_rows` (the band's share), `return_depth_alpha` and inside fixed_capacity; not together with `rest_step` (RuntimeError).  When none
        of the three requires grad the flag changes nothing.  A pose tensor: nerficg_amd.gaussian_splatting.make_raster_settings chains the gradient on to c2w.
        `features`: a (P, C) float32 CUDA tensor of the caller's, 1 <= C <= 256 (semantic or language features, normals, logits, ids, confidences).  The call
        appends one output, feature_map (C, H, W): (image, radii, feature_map), with `return_depth_alpha` (image, radii, depth, alpha, feature_map).
        feature_map[c] = sum w_i features[i, c] with the colour's own blended set and weights w_i = alpha_i T_i, bit for bit, background 0, ACCUMULATED like the
        depth map (divide by alpha for an expectation).  It is differentiable: gradients go to `features` when it requires grad and, through the weights, to every
        geometry input, to `means2D` and -- with `camera_grad` -- to the camera; a feature map that takes no part in the loss counts as a zero gradient (its
        backward launch is skipped, `features.grad` is exact zeros).  The pass is one extra launch on the state the colour pass left (no second preprocess, sort
        or binning) and one more in the backward; image, radii and everything the backward saves are bit for bit those of the call without `features`.  Works with
        every parameter form above, with `tile_rows` (the band's rows and the band's share), `return_depth_alpha`, `camera_grad` and inside fixed_capacity; not
        together with `rest_step` (RuntimeError).  A wrong type, shape, dtype, device or C raises ValueError / RuntimeError naming `features`.
        `absgrad=True`: after backward() the tensor object passed as `means2D` carries `means2D.absgrad`, a (P, 3) float32 tensor on its device: per Gaussian the
        sum over the pixels that blended it of |dL_pixel/dmean2D| (x, y; column 2 zero) -- the addends of `means2D.grad[:, :2]` with the absolute value taken PER
        PIXEL before any sum, in the units of `means2D.grad` (AbsGS; gsplat's absgrad).  The signed sum cancels where a large Gaussian blurs fine texture; this
        one does not: it is the statistic to densify on, with a threshold of its own (it is never smaller than |grad|).  Exact zeros for culled Gaussians and
        those no pixel blended.  Like `.grad` it ACCUMULATES: a backward that finds an `absgrad` of the right shape adds to it (the bands of a partition rendered
        on one leaf sum to the frame's); delete or zero it between steps.  Outputs and every ordinary gradient are those of the call without the flag (same
        per-Gaussian sums; float atomics in another order); without the flag nothing changes.  Works with every parameter form above, with `tile_rows`,
        `return_depth_alpha`, `camera_grad` and inside fixed_capacity (no host read is added); not together with `rest_step` or `features` (RuntimeError).
        `antialiasing=True` (or `antialiasing=True` in the settings, upstream's field; either turns it on): anti-aliased splats, the 2-D filter of Mip-Splatting.
        The 0.3-pixel dilation of the projected covariance adds energy; the flag takes it back: the opacity that is blended is o * comp,
        comp = sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I))) (gsplat's rasterize_mode="antialiased").  Radii, tile lists, conics and colours are bit for bit
        those of the call without the flag, and the call equals, bit for bit, the call without the flag on the compensated opacities; the backward carries the
        gradient through comp to the opacities and, above the floor, to scales, rotations, cov3D_precomp and means3D (`means2D.grad` and `means2D.absgrad` are
        unchanged by it).  Works with every parameter form above, with `tile_rows`, `return_depth_alpha`, `features`, `absgrad`, contributions() and inside
        fixed_capacity; not together with `rest_step` or `camera_grad` (RuntimeError)."""
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = torch.Tensor([])
        self._frame_state = None
        sink: list = []
        previous, _FRAME_STATE_SINK[0] = _FRAME_STATE_SINK[0], sink
        try:
            out = rasterize_gaussians(means3D, means2D, empty if shs is None else shs, empty if colors_precomp is None else colors_precomp, opacities,
                                      empty if scales is None else scales, empty if rotations is None else rotations,
                                      empty if cov3D_precomp is None else cov3D_precomp, self.raster_settings, shs_rest, raw_parameters, rest_step, tile_rows, return_depth_alpha, camera_grad, features, absgrad, antialiasing)
        finally:
            _FRAME_STATE_SINK[0] = previous
        self._frame_state = sink[-1] if sink else None   # what contributions() runs on: references to tensors the forward created anyway
        return out
