"""The index formulas of the colour net's fragment image (tests/colour_frag_image_ref.py) on their own: the image is a permutation of the 7 168 colour
weights -- every weight the fragments read, the head's sixteen rows included --, and the lanes at the edges of every lane group hold the weights that the
fragment builders of csrc/ngp_net.h name for them, restated here one scalar at a time (load_w_frag<false> for slots 0-3, load_w_frag<true> for slots 4-11,
load_w_head_frag for slots 12 and 13) and as a few literal values."""
import numpy as np
import pytest

from tests import colour_frag_image_ref as ref

LANES = (0, 15, 16, 31, 32, 63)


def test_the_image_is_a_permutation_of_the_weights():
    idx = ref.image_indices()
    assert idx.shape == (14, 64, 8) and idx.size == ref.N_WEIGHTS == 7168
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(7168))
    # each layer's slots hold that layer and nothing else
    assert np.array_equal(np.sort(idx[:4].reshape(-1)), np.arange(2048))
    assert np.array_equal(np.sort(idx[4:12].reshape(-1)), np.arange(2048, 6144))
    assert np.array_equal(np.sort(idx[12:].reshape(-1)), np.arange(6144, 7168))
    w = ref.distinct_weights()
    img = ref.image_of(w)
    assert img.dtype == np.float16 and img.nbytes == 14336
    assert np.array_equal(np.sort(img.reshape(-1)), np.sort(w))


def _natural_scalar(f, lane, e):       # load_w_frag<false>(Wc, ld 32, ...): eight consecutive k of the lane half
    mt, s, r, hh = f >> 1, f & 1, lane & 31, lane >> 5
    return (32 * mt + r) * 32 + 16 * s + 8 * hh + e


def _acc_scalar(g, lane, e):           # load_w_frag<true>(Wc + 2048, ld 64, ...): h4 at k 4 hh, then h4 at k 8 + 4 hh of the step
    mt, s, r, hh = g >> 2, g & 3, lane & 31, lane >> 5
    p = 2048 + (32 * mt + r) * 64 + 16 * s
    return p + 4 * hh + e if e < 4 else p + 8 + 4 * hh + (e - 4)


def _head_scalar(ks, lane, e):         # load_w_head_frag(Wc + 6144, ld 64, ...)
    m, kg = lane & 15, lane >> 4
    k = 32 * ks + (e & 3) + 8 * (2 * (kg & 1) + (e >> 2)) + 4 * (kg >> 1)
    return 6144 + m * 64 + k


@pytest.mark.parametrize('slot', range(14))
def test_spot_lanes_of_every_slot(slot):
    idx = ref.image_indices()
    for lane in LANES:
        for e in range(8):
            if slot < 4:
                want = _natural_scalar(slot, lane, e)
            elif slot < 12:
                want = _acc_scalar(slot - 4, lane, e)
            else:
                want = _head_scalar(slot - 12, lane, e)
            assert idx[slot, lane, e] == want, (slot, lane, e)


def test_literal_values():
    idx = ref.image_indices()
    r8 = np.arange(8)
    assert np.array_equal(idx[0, 0], r8)                                  # first layer: row 0, SH coefficients 0-7
    assert np.array_equal(idx[1, 32], 24 + r8)                            # k-step 1 (density features), upper lane half: k 24-31
    assert np.array_equal(idx[3, 63], 63 * 32 + 24 + r8) and idx[3, 63, 7] == 2047
    assert np.array_equal(idx[4, 0], 2048 + np.array([0, 1, 2, 3, 8, 9, 10, 11]))         # second layer: row 0, k-step 0, lower half
    assert np.array_equal(idx[4, 32], 2048 + np.array([4, 5, 6, 7, 12, 13, 14, 15]))      # ... upper half
    assert np.array_equal(idx[7, 31], 2048 + 31 * 64 + 48 + np.array([0, 1, 2, 3, 8, 9, 10, 11]))   # row 31, k-step 3
    assert np.array_equal(idx[8, 0], 2048 + 32 * 64 + np.array([0, 1, 2, 3, 8, 9, 10, 11]))         # m-tile 1: row 32
    assert idx[11, 63, 7] == 6143                                          # the last weight of the second layer
    assert np.array_equal(idx[12, 0], 6144 + np.array([0, 1, 2, 3, 8, 9, 10, 11]))        # head: neuron 0, k-group 0
    assert np.array_equal(idx[12, 16], 6144 + np.array([16, 17, 18, 19, 24, 25, 26, 27]))
    assert np.array_equal(idx[12, 32], 6144 + np.array([4, 5, 6, 7, 12, 13, 14, 15]))
    assert idx[13, 63, 7] == 7167
