"""k_ngp_mlp_composite runs the colour net's first k-step (the SH coefficients of the tile's 64 rays against the first 16 input columns) ONCE per ray
tile and starts every row's colour layer from those accumulators (csrc/ngp_net.hip: mlp_sh_step, mlp_chain with P); k_ngp_mlp keeps the chain that
runs the k-step for every row, because its rows are not ray-ordered.  Both feed the k-step-1 MFMA the same C operand, so the single-pass frame and the
compact-row frame (ARENA_IN_PLACE = False: k_ngp_mlp writes packed records, k_composite_image reads them) must give the same bits -- here with weights
and a table of order one and random fp16 mantissas (the shipped initialisation, U(-1e-4, 1e-4) table entries, would round most differences away), on
tiles whose rays have no sample, one sample and unequal numbers of samples, and on a frame whose last tile column and row are partial."""
import numpy as np
import pytest
import torch

from tests import scenes

pytestmark = pytest.mark.gpu
DEV = 'cuda'
POSE = (3.6, 0.55)      # on both frames below this orbit position leaves rays with exactly one sample (counted on the CPU march; asserted on the device's)


def random_model(device=DEV, seed=7, amps=(4.0, 0.4, 0.6)):
    """the shipped 16 x 2 grid and networks with seeded random parameters of order one: table U(-4, 4), density net U(-0.4, 0.4), colour net
    U(-0.6, 0.6) -- pre-activations of order one at every layer.  On the CPU oracle this scene has densities from 0.1 to above 100 (rays that saturate after
    a few rows next to rays that never do, so tiles retire early and late), sample colours with a standard deviation of 0.43 and 660 translucent pixels"""
    from nerficg_amd.instant_ngp import InstantNGPModel
    model = InstantNGPModel(RANDOM_SEED=seed, device=device)
    g = torch.Generator().manual_seed(seed)
    u = lambda n, amp: ((torch.rand(n, generator=g) * 2 - 1) * amp).to(device)
    with torch.no_grad():
        n_mlp = model.n_params_encoding_mlp
        model.encoding_xyz.params[:n_mlp] = u(n_mlp, amps[1])
        model.encoding_xyz.params[n_mlp:] = u(model.encoding_xyz.params.numel() - n_mlp, amps[0])
        model.color_mlp_with_encoding.params.copy_(u(model.color_mlp_with_encoding.params.numel(), amps[2]))
        model.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.35, 1)).to(device))
    return model


@pytest.fixture(scope='module')
def renderers():
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    model = random_model()
    fused, rows = InstantNGPRenderer(model), InstantNGPRenderer(model)
    rows.ARENA_IN_PLACE = False       # compact rows: k_grid_encode / k_ngp_mlp (the k-step per row), then k_composite_image
    return fused, rows


def _frame(renderer, cam, pose, **kw):
    r = renderer.render_image_fused(cam, pose, return_stats=True, early_termination=False, **kw)
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items() if k in ('rgb', 'alpha', 'depth', 'n_samples', 'n_rows')}


def _tile_counts(renderer, w, h):
    """samples per ray of the last frame, [tile][8 x 8 pixels], 0 for the rays of a partial tile that lie outside the picture"""
    (ws,) = renderer._fused_ws.values()
    tx, ty = (w + 7) // 8, (h + 7) // 8
    cnt = ws['ray_cnt'].cpu().numpy().reshape(ty, tx, 8, 8)
    py = np.arange(ty)[:, None, None, None] * 8 + np.arange(8)[None, None, :, None]
    px = np.arange(tx)[None, :, None, None] * 8 + np.arange(8)[None, None, None, :]
    return np.where((px < w) & (py < h), cnt, 0).reshape(-1, 64)


@pytest.mark.parametrize('w,h', [(64, 48), (61, 45)])
def test_single_pass_frame_equals_the_compact_row_frame(renderers, w, h):
    from tests.test_gpu_render_parity import make_camera
    fused, rows = renderers
    cam = make_camera(w, h, bg=(0.2, 0.5, 0.7))
    pose = scenes.orbit_pose(*POSE, scenes.LEGO_RADIUS)
    want = _frame(rows, cam, pose)
    got = _frame(fused, cam, pose)
    cnt = _tile_counts(fused, w, h)
    # the tiles this test is about: no sample at all, a ray with exactly one sample, rays of one tile with different numbers of samples
    assert cnt.shape[0] == 48 and (cnt.max(1) == 0).any() and (cnt == 1).any() and (cnt.max(1) != cnt.min(1)).sum() >= 30
    assert got['n_samples'] == want['n_samples'] == int(cnt.sum()) and got['n_rows'] == want['n_rows']
    # a picture that would show a wrong accumulator: translucent and opaque pixels, colours all over the range
    a = want['alpha']
    assert int(((a > 0.05) & (a < 0.95)).sum()) > 50 and float(a.max()) > 0.99
    lit = want['rgb'][a > 0.5]
    assert float(lit.std()) > 0.05 and torch.unique(lit).numel() > 1000
    for k in ('rgb', 'alpha', 'depth'):
        assert torch.equal(got[k], want[k]), (w, h, k)


def test_a_tile_shard_equals_the_compact_row_shard(renderers):
    """tiles [13, 37) of the 61 x 45 frame: the chunk's first tile is not tile 0, so ray_sh and the arena are addressed behind an offset"""
    from tests.test_gpu_render_parity import make_camera
    fused, rows = renderers
    cam = make_camera(61, 45, bg=(1.0, 1.0, 1.0))
    pose = scenes.orbit_pose(*POSE, scenes.LEGO_RADIUS)
    want = _frame(rows, cam, pose, tile_begin=13, n_tiles=24)
    got = _frame(fused, cam, pose, tile_begin=13, n_tiles=24)
    assert got['n_samples'] == want['n_samples'] > 0
    for k in ('rgb', 'alpha', 'depth'):
        assert torch.equal(got[k], want[k]), k
