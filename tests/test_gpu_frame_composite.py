"""The single-pass frame composites inside its MLP kernel (nrc_ngp_render_frame: whole ray tiles per wave, longest first, chunks of whole
tiles under a row budget).  Its pictures must equal the separate compositor's (k_composite_image, reached through the compact-row frame,
ARENA_IN_PLACE = False) and the slab order's (k_composite_layers) bit for bit, with the same row and sample counts -- whatever the number of
chunks the row budget cuts the frame into, on shards, on cameras whose size is not a multiple of the 8 x 8 tile, with 1 and 3 cascades."""
import pytest
import torch

from tests import scenes

DEV = 'cuda'


def _frame(renderer, cam, pose, **kw):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in renderer.render_image_fused(cam, pose, return_stats=True, **kw).items()}


def _same(a, b, what):
    assert a['n_rows'] == b['n_rows'] and a['n_samples'] == b['n_samples'] and a['n_samples'] > 0, what
    for key in ('rgb', 'alpha', 'depth'):
        assert torch.equal(a[key], b[key]), (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize('cascades', [1, 3])
def test_fused_frame_equals_the_separate_compositor(cascades):
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    if cascades > 1:
        from tests.test_gpu_garden_parity import garden_model
        model, radius, esf = garden_model(), 1.15, True
        assert model.cascades == cascades
    else:
        model, radius, esf = make_model(table_amp=4.0), scenes.LEGO_RADIUS, False
    fused = InstantNGPRenderer(model, EXPONENTIAL_STEPS=esf)
    small = InstantNGPRenderer(model, EXPONENTIAL_STEPS=esf)
    small.FRAME_ROW_BUDGET = 2 * small.MAX_SAMPLES      # the smallest budget: many chunks of whole ray tiles
    ref = InstantNGPRenderer(model, EXPONENTIAL_STEPS=esf)
    ref.ARENA_IN_PLACE = False                          # compact rows: encode / MLP kernels, then k_composite_image
    for cam in (make_camera(99, 70, bg=(0.2, 0.5, 0.7)), make_camera(61, 45, bg=(1.0, 1.0, 1.0))):
        n_tiles = fused.n_image_tiles(cam)
        for k in range(3):
            pose = scenes.orbit_pose(0.3 + 1.1 * k, 0.1 + 0.15 * k, radius)
            for t0, nt in ((0, None), (n_tiles // 4, n_tiles // 2)):
                want = _frame(ref, cam, pose, tile_begin=t0, n_tiles=nt, early_termination=False)
                got = _frame(fused, cam, pose, tile_begin=t0, n_tiles=nt, early_termination=False)
                _same(got, want, ('default budget', cam.width, k, t0))
                if t0 == 0 and k == 0 and cam.width == 99:
                    assert got['n_rows'] > 2 * small.FRAME_ROW_BUDGET, 'the small budget must cut this frame into several chunks'
                _same(_frame(small, cam, pose, tile_begin=t0, n_tiles=nt, early_termination=False), want, ('small budget', cam.width, k, t0))
                _same(_frame(fused, cam, pose, tile_begin=t0, n_tiles=nt, early_termination=True), want, ('slab order', cam.width, k, t0))


@pytest.mark.gpu
def test_fused_frame_shards_compose_under_a_small_budget():
    """Contiguous tile shards rendered through the fused frame, each cut into chunks by a small row budget, compose into the whole frame."""
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from nerficg_amd.parallel import shard_range
    from tests.test_gpu_render_parity import make_camera, make_model
    model = make_model()
    renderer = InstantNGPRenderer(model)
    cam = make_camera(83, 77, bg=(0.3, 0.3, 0.3))
    pose = scenes.orbit_pose(1.7, 0.25, scenes.LEGO_RADIUS)
    whole = _frame(renderer, cam, pose, early_termination=False)
    renderer.FRAME_ROW_BUDGET = 3 * renderer.MAX_SAMPLES
    n_tiles = renderer.n_image_tiles(cam)
    out = {k: torch.full_like(whole[k], -1.0) for k in ('rgb', 'alpha', 'depth')}
    for rank in range(3):
        b, e = shard_range(n_tiles, rank, 3)
        renderer.render_image_fused(cam, pose, tile_begin=b, n_tiles=e - b, out=out, early_termination=False)
    for key in out:
        assert torch.equal(out[key], whole[key]), key


def test_frame_workspace_validates_the_row_budget():
    """nrc_ngp_render_frame_ws_bytes: a budget below two tiles' worth of rows is refused; more chunks never need less workspace per row."""
    from nerficg_amd import _lib
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    assert lib.nrc_ngp_render_frame_ws_bytes(10_000, 100, 1024, 2047) < 0
    assert lib.nrc_ngp_render_frame_ws_bytes(-1, 100, 1024, 0) < 0
    one = lib.nrc_ngp_render_frame_ws_bytes(10_000, 100, 1024, 0)
    cut = lib.nrc_ngp_render_frame_ws_bytes(10_000, 100, 1024, 2048)
    assert one >= 10_000 * 64 * 64 and 2048 * 64 * 64 <= cut < one
