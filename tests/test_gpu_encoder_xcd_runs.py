"""k_grid_encode<SRC_TILED> deals its workgroups to the eight XCDs in RUNS of 8 G workgroups: inside a run XCD x takes the G consecutive workgroups
behind x G, and what is left behind the last whole run is split in eight the same way (nrc_ngp_set_encoder_xcd_run; the library's default G is sized
for an 800 x 800 frame, so a small frame is one short run and never meets a run boundary on its own).

Which workgroup encodes a slot changes neither the slot nor a value: with G = 4, 8 and 12 a small frame -- several whole runs plus a remainder that is
no whole run, in ONE encode / MLP round -- must paint bit for bit the picture of the default, under each of the three pose-dependent brick shapes
(the brick remapping permutes the slots of a block of 1024 = 4 workgroups, so the two permutations compose)."""
import numpy as np
import pytest
import torch

from tests import scenes

DEV = 'cuda'
RUNS = (4, 8, 12)


def _look(fwd, down):
    fwd, down = np.asarray(fwd, np.float64), np.asarray(down, np.float64)
    fwd /= np.linalg.norm(fwd)
    right = np.cross(down, fwd); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, -1.3 * fwd
    return c2w


# one pose per brick shape the renderer chooses (InstantNGPRenderer._frame_constants): 4 x 4 x 4, 4 x 2 x 8, 8 x 2 x 4
POSES = {'columns along x': (_look((0.1, 0.2, 1.0), (1.0, 0.1, 0.0)), (2, 2)), 'looking down x': (_look((1.0, 0.05, 0.1), (0.0, 1.0, 0.0)), (2, 1)),
         'rows along x': (_look((0.0, 0.3, 1.0), (0.0, 1.0, 0.0)), (3, 1))}


@pytest.mark.gpu
@pytest.mark.parametrize('pose', sorted(POSES))
def test_every_xcd_run_length_paints_the_default_picture(pose):
    from nerficg_amd import _lib
    from nerficg_amd.instant_ngp import InstantNGPRenderer
    from tests.test_gpu_render_parity import make_camera, make_model
    lib = _lib.load()
    model = make_model()
    with torch.no_grad():   # a ball of radius 0.15: about 3 x 3 of the 8 x 6 ray tiles carry rows, so that the frame stays below the row budget of one round
        model.occupancy_bitfield.copy_(torch.from_numpy(scenes.sphere_bitfield(128, 0.5, 0.15, 1)).to(DEV))
    cam = make_camera(60, 45)
    c2w, shape = POSES[pose]
    r = InstantNGPRenderer(model)
    r.FRAME_ROW_BUDGET = 2 * r.MAX_SAMPLES
    assert r._frame_constants(cam, c2w)['enc_shape'] == shape
    try:
        assert lib.nrc_ngp_set_encoder_xcd_run(0) == 0
        out = r.render_image_fused(cam, c2w, early_termination=False, return_stats=True)
        want = {k: out[k].clone() for k in ('rgb', 'alpha', 'depth')}
        rows, slots = out['n_rows'], out['n_slots']
        # one round (no chunking of the frame), and for every G at least one whole run followed by a remainder that is no whole run
        assert 0 < rows <= r.FRAME_ROW_BUDGET
        # the picture is not an empty one: the ball's disc (radius ~ 10 of 60 pixels: a tenth of the frame) has alpha, the rest has none.  (No bound on how
        # opaque: the chords of this ball are 0.3 at the most, the random-init model reaches alpha ~ 0.3 on them.)
        assert float((want['alpha'] > 0).float().mean()) > 0.05 and float(want['alpha'].max()) > 0.1 and float(want['alpha'].min()) == 0.0
        for g in RUNS:
            assert slots > 8 * g * 256 and slots % (8 * g * 256) != 0, (g, slots)
            assert lib.nrc_ngp_set_encoder_xcd_run(g) == 0
            # the features of the frame before are still in the workspace, and they are the right ones: overwrite them (fp16 1.06 in every feature), so that a
            # slot no workgroup encodes shows in the picture
            next(iter(r._fused_ws.values()))['fws'].fill_(0x3C)
            got = r.render_image_fused(cam, c2w, early_termination=False, return_stats=True)
            assert got['n_rows'] == rows
            for k in want:
                assert torch.equal(got[k], want[k]), (pose, g, k)
    finally:
        lib.nrc_ngp_set_encoder_xcd_run(0)
        lib.nrc_ngp_set_encoder_shape(-1, -1)


def test_the_setter_takes_zero_or_a_positive_multiple_of_four():
    """0 = the library's default; a run must keep blocks of 1024 slots (4 workgroups) whole; the value is a per-thread setting and is put back to the default."""
    from nerficg_amd import _lib
    lib = _lib.load()
    try:
        for ok in (4, 8, 12, 256, 1024, 4096, 1 << 24, 0):
            assert lib.nrc_ngp_set_encoder_xcd_run(ok) == 0, ok
        for bad in (-1, -4, 1, 2, 3, 5, 6, 7, 10, 4097, (1 << 24) + 4, 2 ** 31 - 1):
            assert lib.nrc_ngp_set_encoder_xcd_run(bad) == -1, bad
    finally:
        lib.nrc_ngp_set_encoder_xcd_run(0)
