"""Where the density-encoder form of k_grid_encode stores what (nerficg_amd/csrc/ngp_net.hip), stated again in Python.

Slot j of a chunk owns 32 bytes: density features 8 hh .. 8 hh + 7 (fp16) in the 16-byte vector  64 (j >> 5) + 32 hh + (j & 31),  hh = 0, 1 -- the
1 KB record of the 32-sample tile j >> 5 in the lane order of the MFMA wave that reads it.  The encoder's wave does not hold a tile of 32 consecutive
slots: lane l of wave w of a block of 1024 slots gathers for the slot its brick shape deals it, the chain runs on tile v = lanes 32 v .. 32 v + 31, and
lane 32 hh + r ends up with half hh of the sample of lane 32 v + r, whose slot it gets from that lane.  Every 16-byte vector of the range must be
written exactly once, whatever the shape."""
import numpy as np
import pytest

TILE_W, TILE_W_LOG2, TILE_H = 8, 3, 8
SHAPES = {'8x2x4': (3, 1), '4x4x4': (2, 2), '4x2x8': (2, 1)}
SLOTS = 2048


def record_vector(slot, hh):
    """index of the 16-byte vector that holds density features 8 hh .. 8 hh + 7 of `slot`"""
    return (slot >> 5) * 64 + 32 * hh + (slot & 31)


def brick_slot(block, w, l, lu, lv):
    """the slot that lane l of wave w of a block of 1024 slots encodes (the remapping of k_grid_encode for a brick of 2^lu x 2^lv pixels)"""
    ls = 6 - lu - lv
    iu, iv, i_s = l & ((1 << lu) - 1), (l >> lu) & ((1 << lv) - 1), l >> (lu + lv)
    gu, gv, gs = w & ((TILE_W >> lu) - 1), (w >> (TILE_W_LOG2 - lu)) & ((TILE_H >> lv) - 1), w >> (6 - lu - lv)
    return 1024 * block + (((gs << ls) + i_s) << 6) + TILE_W * ((gv << lv) + iv) + (gu << lu) + iu


def encoder_stores(lu, lv, slots):
    """(vector index, slot, half) of every 16-byte store the encoder's waves issue for `slots` slots"""
    out = []
    for block in range(slots // 1024):
        for w in range(16):
            own = [brick_slot(block, w, l, lu, lv) for l in range(64)]
            for v in range(2):            # MFMA tile v = the samples on lanes 32 v .. 32 v + 31
                for lane in range(64):    # lane 32 hh + r stores half hh of the sample on lane 32 v + r
                    hh, r = lane >> 5, lane & 31
                    slot = own[32 * v + r]
                    out.append((record_vector(slot, hh), slot, hh))
    return out


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_the_records_tile_the_range_exactly(shape):
    lu, lv = SHAPES[shape]
    # the remapping itself is a permutation of the block's slots
    assert sorted(brick_slot(b, w, l, lu, lv) for b in range(SLOTS // 1024) for w in range(16) for l in range(64)) == list(range(SLOTS))
    stores = encoder_stores(lu, lv, SLOTS)
    vectors = np.array([s[0] for s in stores])
    assert len(vectors) == 2 * SLOTS
    assert np.array_equal(np.sort(vectors), np.arange(2 * SLOTS))   # a bijection onto [0, 32 B x slots) in 16-byte units
    # ... and the reader's view: lane 32 hh + r of the MLP wave's tile T loads vector 64 T + lane and must find half hh of slot 32 T + r
    held = {vec: (slot, hh) for vec, slot, hh in stores}
    for T in range(SLOTS // 32):
        for lane in range(64):
            assert held[64 * T + lane] == (32 * T + (lane & 31), lane >> 5)


def test_the_partner_lane_is_the_other_tile():
    """a lane's partner in the slot exchange is lane ^ 32: for every shape the partner's slot lies in another row of the layout (lu + lv <= 5 puts lane
    bit 5 into the step index), so the two halves of a sample's record are written by two different lanes of one wave"""
    for lu, lv in SHAPES.values():
        for w in range(16):
            for l in range(32):
                a, b = brick_slot(0, w, l, lu, lv), brick_slot(0, w, l + 32, lu, lv)
                assert a >> 6 != b >> 6 and (a & 63) == (b & 63)
