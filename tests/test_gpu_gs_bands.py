"""GPU: one 3DGS view rendered and differentiated as bands of 16-pixel tile rows (the rasterizer's `tile_rows`, C ABI nrc_gs_*_band).

The depth pre-sort runs over all P Gaussians and the blend of a tile depends only on that tile's list and the splat records, so a band reproduces its part of
the whole frame EXACTLY: pixel rows, n_contrib, final_T and the per-tile lists are compared with torch.equal.  The backward is linear in the per-Gaussian
records, so the bands' gradient shares must add up to the whole-frame gradient up to the order of the f32 additions: the project's gradient gate, 2e-3 of the
tensor's own max magnitude (tests/test_gpu_fullsize_properties.py, tests/test_gpu_gs_parity.py)."""
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'
GRAD_NAMES = ('means3D', 'means2D', 'shs', 'opacities', 'scales', 'rotations')


def _settings(w, h, pose=(0.5, 0.3, 3.0)):
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizationSettings
    from tests import scenes
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(*pose))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return GaussianRasterizationSettings(image_height=h, image_width=w, tanfovx=cam['tanfovx'], tanfovy=cam['tanfovy'], bg=torch.tensor([0.1, 0.2, 0.3], device=DEV),
                                         scale_modifier=1.0, viewmatrix=T(cam['viewmatrix']), projmatrix=T(cam['projmatrix']), sh_degree=3, campos=T(cam['campos']),
                                         prefiltered=False, debug=False)


def _small_scene(n=3000, raw=False):
    from tests import scenes
    sc = scenes.gs_random_scene(n, seed=1, extent=1.0, log_scale_mean=math.log(0.05))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = dict(means3D=T(sc['means3D']), shs=T(sc['shs']), opacities=T(sc['opacities'])[:, None].contiguous(), scales=T(sc['scales']), rotations=T(sc['rotations']))
    if raw:   # the model's own tensors: logits, log-scales, unnormalised quaternions, SH split into dc + rest
        t['opacities'] = torch.special.logit(t['opacities'].clamp(1e-4, 1 - 1e-4))
        t['scales'] = t['scales'].log()
        t['rotations'] = t['rotations'] * 1.7
    return t


def _render(rs, t, tile_rows=None, grad=False, raw=False):
    """One call of the drop-in module.  Returns the image, radii, the leaves (with .grad after backward) and the rasterizer state of the call."""
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer, last_band_mask
    a = {k: v.detach().clone().requires_grad_(True) for k, v in t.items()}
    m2d = torch.zeros_like(a['means3D'], requires_grad=True)
    kw = dict(tile_rows=tile_rows) if tile_rows is not None else {}
    if raw:
        kw.update(shs=a['shs'][:, :1].contiguous(), shs_rest=a['shs'][:, 1:].contiguous(), raw_parameters=True)
    else:
        kw.update(shs=a['shs'])
    color, radii = GaussianRasterizer(rs)(means3D=a['means3D'], means2D=m2d, opacities=a['opacities'], scales=a['scales'], rotations=a['rotations'], **kw)
    st = color.grad_fn.debug_state
    state = dict(point_list=st['point_list'], ranges=st['ranges'].view(-1, 2).long(), n_contrib=st['n_contrib'], final_T=st['final_T'],
                 counts=[int(v) for v in st['num_rendered'].tolist()], mask=last_band_mask())
    a['means2D'] = m2d
    return color, radii, a, state


def _partitions(gy):
    one_row = [(y, 1) for y in range(gy)]
    two = [(0, gy // 2), (gy // 2, gy - gy // 2)]
    a, b = max(1, gy // 6), max(2, gy // 2)
    three = [(0, a), (a, b - a), (b, gy - b)]                     # uneven
    return {'one_row_bands': one_row, 'two_bands': two, 'three_uneven_bands': three, 'single_full_band': [(0, gy)]}


def _check_band_against_frame(whole, band_out, band, W, H, gx, gy):
    """Everything the issue asks of ONE band call against the whole-frame call."""
    color_w, radii_w, _, st_w = whole
    color_b, radii_b, _, st_b = band_out
    y0, y1 = min(H, 16 * band[0]), min(H, 16 * (band[0] + band[1]))
    assert torch.equal(radii_b, radii_w)
    assert torch.equal(color_b[:, y0:y1], color_w[:, y0:y1]), f'band {band}: pixel rows differ from the whole frame'
    assert not color_b[:, :y0].any() and not color_b[:, y1:].any(), f'band {band}: the image is zero outside the band'
    for name in ('n_contrib', 'final_T'):
        assert torch.equal(st_b[name].view(H, W)[y0:y1], st_w[name].view(H, W)[y0:y1]), (band, name)
    rb, rw = st_b['ranges'].cpu(), st_w['ranges'].cpu()
    pb, pw = st_b['point_list'].cpu(), st_w['point_list'].cpu()
    in_band = torch.zeros(gy, gx, dtype=torch.bool)
    in_band[band[0]:band[0] + band[1]] = True
    in_band = in_band.flatten()
    assert bool((rb[~in_band, 1] == rb[~in_band, 0]).all()), f'band {band}: a tile outside the band has a list'
    assert torch.equal((rb[:, 1] - rb[:, 0])[in_band], (rw[:, 1] - rw[:, 0])[in_band]), f'band {band}: list lengths'
    for tile in torch.nonzero(in_band).flatten().tolist():
        assert torch.equal(pb[rb[tile, 0]:rb[tile, 1]], pw[rw[tile, 0]:rw[tile, 1]]), f'band {band}: list of tile {tile}'
    assert st_b['counts'][0] == int((rb[:, 1] - rb[:, 0]).sum())
    return st_b['counts'][0]


W_SMALL, H_SMALL = 200, 139          # gy = 9 tile rows, the last one 11 pixel rows high


@pytest.mark.parametrize('variant', ['plain', 'raw_split_sh', 'fixed_capacity'])
def test_small_scene_bands_reproduce_the_frame_bit_for_bit(variant):
    import contextlib
    from nerficg_amd.diff_gaussian_rasterization import fixed_capacity
    raw = variant == 'raw_split_sh'
    rs, t = _settings(W_SMALL, H_SMALL), _small_scene(raw=raw)
    gx, gy = (W_SMALL + 15) // 16, (H_SMALL + 15) // 16
    assert H_SMALL % 16 and gy == 9
    probe = _render(rs, t, raw=raw)
    n_whole = probe[3]['counts'][0]
    assert n_whole > 5000 and int((probe[1] > 0).sum()) > 1000
    cap = fixed_capacity(n_whole + 1024, 0) if variant == 'fixed_capacity' else contextlib.nullcontext()      # a capacity that drops nothing
    with cap:
        whole = _render(rs, t, raw=raw)
        assert whole[3]['counts'][0] == n_whole and torch.equal(whole[0], probe[0])
        parts = _partitions(gy) if variant == 'plain' else {k: v for k, v in _partitions(gy).items() if k in ('three_uneven_bands', 'single_full_band')}
        for name, bands in parts.items():
            assert sum(n for _, n in bands) == gy
            total, composed = 0, torch.zeros_like(whole[0])
            for band in bands:
                out = _render(rs, t, tile_rows=band, raw=raw)
                total += _check_band_against_frame(whole, out, band, W_SMALL, H_SMALL, gx, gy)
                composed += out[0]
            assert total == n_whole, (name, total, n_whole)           # the bands' instance counts add up exactly
            assert torch.equal(composed, whole[0]), name               # the band images sum to the frame (zeros elsewhere)


def test_whole_frame_path_is_unchanged_by_the_full_band():
    rs, t = _settings(W_SMALL, H_SMALL), _small_scene()
    gy = (H_SMALL + 15) // 16
    a, b = _render(rs, t), _render(rs, t, tile_rows=(0, gy))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[3]['ranges'], b[3]['ranges']) and torch.equal(a[3]['point_list'], b[3]['point_list'])
    assert torch.equal(a[3]['n_contrib'], b[3]['n_contrib']) and torch.equal(a[3]['final_T'], b[3]['final_T']) and a[3]['counts'] == b[3]['counts']
    assert a[3]['mask'] is None and torch.equal(b[3]['mask'], b[1] > 0)      # every visible Gaussian touches the band that is the frame


def test_tile_rows_out_of_range_and_rest_step_are_refused():
    rs, t = _settings(W_SMALL, H_SMALL), _small_scene()
    for bad in ((-1, 2), (0, 0), (8, 2), (9, 1)):
        with pytest.raises(ValueError, match='tile_rows'):
            _render(rs, t, tile_rows=bad)
    from nerficg_amd.diff_gaussian_rasterization import GaussianRasterizer
    with pytest.raises(RuntimeError, match='partial gradient'):      # the in-backward Adam step of f_rest has no band form
        GaussianRasterizer(rs)(means3D=t['means3D'], means2D=torch.zeros_like(t['means3D']), opacities=t['opacities'], shs=t['shs'][:, :1].contiguous(),
                               shs_rest=t['shs'][:, 1:].contiguous(), scales=t['scales'], rotations=t['rotations'], rest_step=object(), tile_rows=(0, 4))


def _band_gradient_sum(rs, t, bands, g, whole_grads):
    """Backward of every band with the SAME full-frame dL_dpix; returns the sums of the shares and checks the exact zeros outside each band's mask."""
    sums = None
    for band in bands:
        color, radii, leaves, st = _render(rs, t, tile_rows=band)
        color.backward(g)
        mask = st['mask']
        assert mask.dtype == torch.bool and mask.shape == radii.shape and not bool((mask & ~(radii > 0)).any())
        share = {k: leaves[k].grad for k in GRAD_NAMES}
        for k, v in share.items():
            assert v is not None and not bool(v[~mask].ne(0).any()), f'band {band}: {k} has a non-zero row outside the band mask'
        sums = {k: v.clone() for k, v in share.items()} if sums is None else {k: sums[k] + share[k] for k in sums}
    errs = {}
    for k in GRAD_NAMES:
        scale = float(whole_grads[k].abs().max())
        assert scale > 0, k
        errs[k] = float((sums[k] - whole_grads[k]).abs().max()) / scale
    return errs


def test_small_scene_band_gradients_sum_to_the_frame_gradient():
    from nerficg_amd import parallel
    rs, t = _settings(W_SMALL, H_SMALL), _small_scene()
    gy = (H_SMALL + 15) // 16
    g = torch.randn(3, H_SMALL, W_SMALL, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    color, _, leaves, _ = _render(rs, t)
    color.backward(g)
    whole = {k: leaves[k].grad.clone() for k in GRAD_NAMES}
    errs = _band_gradient_sum(rs, t, [parallel.tile_row_band(gy, r, 8) for r in range(8)], g, whole)
    print('small scene, 8 bands: max |sum of shares - whole| / max |whole| =', errs)
    assert all(e <= 2e-3 for e in errs.values()), errs


@pytest.fixture(scope='module')
def big():
    import bench
    return {(w, h): bench.build_gs_scene(DEV, n=1_000_000, seed=0, w=w, h=h) for w, h in ((1297, 840), (1600, 1060))}


def _big_tensors(gs):
    return {k: gs['tensors'][k] for k in ('means3D', 'shs', 'opacities', 'scales', 'rotations')}


@pytest.mark.parametrize('size', [(1297, 840), (1600, 1060)])
def test_full_size_eight_bands_compose_the_frame(big, size):
    from nerficg_amd import parallel
    w, h = size
    gs = big[size]
    rs, t = gs['rast'].raster_settings, _big_tensors(gs)
    gx, gy = (w + 15) // 16, (h + 15) // 16
    whole = _render(rs, t)
    total, composed = 0, torch.zeros_like(whole[0])
    for r in range(8):
        band = parallel.tile_row_band(gy, r, 8)
        out = _render(rs, t, tile_rows=band)
        total += _check_band_against_frame(whole, out, band, w, h, gx, gy)
        composed += out[0].detach()
    assert total == whole[3]['counts'][0] > 1_000_000
    assert torch.equal(composed, whole[0].detach())


def test_full_size_band_gradients_sum_to_the_frame_gradient(big):
    from nerficg_amd import parallel
    w, h = 1600, 1060
    gs = big[(w, h)]
    rs, t = gs['rast'].raster_settings, _big_tensors(gs)
    gy = (h + 15) // 16
    g = torch.randn(3, h, w, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    color, _, leaves, _ = _render(rs, t)
    color.backward(g)
    whole = {k: leaves[k].grad.clone() for k in GRAD_NAMES}
    errs = _band_gradient_sum(rs, t, [parallel.tile_row_band(gy, r, 8) for r in range(8)], g, whole)
    print('1 M Gaussians @ 1600x1060, 8 bands: max |sum of shares - whole| / max |whole| =', errs)
    assert all(e <= 2e-3 for e in errs.values()), errs


# ---------------------------------------------------------------------------------------------------- one step, end to end
STEP_CHILD = r'''
import json, math, os, sys
sys.path.insert(0, os.environ['NRC_ROOT'])
import numpy as np
import torch
from nerficg_amd import parallel
from nerficg_amd.gaussian_splatting import Gaussians, PerspectiveCamera, render_image_training, band_parallel_training_step, training_loss
from tests import scenes
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
backend = os.environ['NRC_BACKEND']
rank, world = parallel.init_distributed(backend, dev if backend == 'nccl' else None, single_rank_group=True)
if world == 1:
    parallel.single_rank_collectives(True)
W, H, P = 200, 139, 3000
sc = scenes.gs_random_scene(P, seed=1, extent=1.0, log_scale_mean=math.log(0.05))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
opac = torch.special.logit(T(sc['opacities']).clamp(1e-4, 1 - 1e-4))[:, None].contiguous()


def model():
    return Gaussians(T(sc['means3D']), T(sc['scales']).log(), T(sc['rotations']) * 1.3, opac.clone(), T(sc['shs'])[:, :1].contiguous(), T(sc['shs'])[:, 1:].contiguous(), 3)


cam = PerspectiveCamera(W, H, 1.2 * W, 1.2 * W, background_color=torch.tensor([0.1, 0.2, 0.3]))
c2w = scenes.orbit_pose(0.5, 0.3, 3.0)
target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
names = ('_positions', '_features_dc', '_features_rest', '_opacities', '_scales', '_rotations')

single = model()
out1 = render_image_training(single, cam, c2w)
training_loss(out1['rgb'], target).backward()
ref = {n: getattr(single, n).grad.clone() for n in names}
ref['viewspace'] = out1['viewspace_points'].grad.clone()

banded = model()
outb = band_parallel_training_step(banded, cam, c2w, lambda image: training_loss(image, target))
got = {n: getattr(banded, n).grad for n in names}
got['viewspace'] = outb['viewspace_points'].grad
torch.cuda.synchronize()
res = dict(rank=rank, world=world, band=list(outb['band']), image_equal=bool(torch.equal(outb['rgb'], out1['rgb'].detach())),
           radii_equal=bool(torch.equal(outb['radii'], out1['radii'])), loss=[float(training_loss(out1['rgb'].detach(), target)), float(outb['loss'])],
           errs={k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref})
try:
    render_image_training(banded, cam, c2w, fuse_rest_step=True, band=(0, 4))
    res['fused_refused'] = ''
except RuntimeError as e:
    res['fused_refused'] = str(e)
if torch.distributed.is_initialized():
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
print('RESULT ' + json.dumps(res))
'''


def _spawn(tmp_path, world, backend):
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    script = tmp_path / 'band_step_child.py'
    script.write_text(STEP_CHILD)
    procs = []
    for r in range(world):
        env = dict(os.environ, NRC_ROOT=str(ROOT), NRC_BACKEND=backend, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK='0',
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for pr in procs:
        try:
            so, se = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert pr.returncode == 0, so[-2000:] + se[-4000:]
        outs.append(json.loads([ln for ln in so.splitlines() if ln.startswith('RESULT ')][-1][len('RESULT '):]))
    return outs


@pytest.mark.parametrize('world,backend', [(1, 'nccl'), (2, 'gloo')])
def test_band_parallel_training_step_matches_the_single_gpu_step(tmp_path, world, backend):
    """The band-parallel training render of one view on a one-rank RCCL group (every collective issued) and on two gloo ranks sharing the GPU: after the
    exchange every rank holds the single-GPU gradients (2e-3 of each tensor's scale), the gathered image is the single-GPU image bit for bit, and
    band= together with the fused f_rest step raises."""
    outs = _spawn(tmp_path, world, backend)
    assert sorted(o['rank'] for o in outs) == list(range(world))
    gy = (139 + 15) // 16
    from nerficg_amd import parallel
    for o in outs:
        print(o)
        assert o['world'] == world and tuple(o['band']) == parallel.tile_row_band(gy, o['rank'], world)
        assert o['image_equal'] and o['radii_equal'] and abs(o['loss'][0] - o['loss'][1]) <= 1e-5 * abs(o['loss'][0])      # (the loss reduction adds in any order)
        assert all(e <= 2e-3 for e in o['errs'].values()), o['errs']
        assert 'partial gradient' in o['fused_refused'], o['fused_refused']
