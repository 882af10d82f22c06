"""The index formulas of the density net's fragment image (tests/density_frag_image_ref.py) on their own: the image is a permutation of the 3 072 weights,
and the lanes at the edges of every lane group hold the weights that the two fragment builders of csrc/ngp_net.h name for them, restated here one scalar
at a time (load_w_frag<false> for slots 0-3, load_w_head_frag for slots 4 and 5) and as a few literal values."""
import numpy as np
import pytest

from tests import density_frag_image_ref as ref

LANES = (0, 15, 16, 31, 32, 63)


def test_the_image_is_a_permutation_of_the_weights():
    idx = ref.image_indices()
    assert idx.shape == (6, 64, 8) and idx.size == ref.N_WEIGHTS == 3072
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(3072))
    # the first-layer slots hold the first layer, the head slots the head, and nothing else
    assert np.array_equal(np.sort(idx[:4].reshape(-1)), np.arange(2048))
    assert np.array_equal(np.sort(idx[4:].reshape(-1)), np.arange(2048, 3072))
    w = ref.distinct_weights()
    img = ref.image_of(w)
    assert img.dtype == np.float16 and img.nbytes == 6144
    assert np.array_equal(np.sort(img.reshape(-1)), np.sort(w))


def _first_layer_scalar(f, lane, e):
    mt, s, r, hh = f >> 1, f & 1, lane & 31, lane >> 5
    row = 32 * mt + r
    return row * 32 + 16 * s + 8 * hh + e


def _head_scalar(ks, lane, e):
    m, kg = lane & 15, lane >> 4
    k = 32 * ks + (e & 3) + 8 * (2 * (kg & 1) + (e >> 2)) + 4 * (kg >> 1)
    return 64 * 32 + m * 64 + k


@pytest.mark.parametrize('slot', range(6))
def test_spot_lanes_of_every_slot(slot):
    idx = ref.image_indices()
    for lane in LANES:
        for e in range(8):
            want = _first_layer_scalar(slot, lane, e) if slot < 4 else _head_scalar(slot - 4, lane, e)
            assert idx[slot, lane, e] == want, (slot, lane, e)


def test_literal_values():
    idx = ref.image_indices()
    r8 = np.arange(8)
    assert np.array_equal(idx[0, 0], r8)                       # row 0, k 0-7
    assert np.array_equal(idx[0, 32], 8 + r8)                  # row 0, k 8-15: the upper lane half
    assert np.array_equal(idx[1, 0], 16 + r8)                  # k-step 1
    assert np.array_equal(idx[0, 31], 31 * 32 + r8)            # row 31
    assert np.array_equal(idx[2, 31], 63 * 32 + r8)            # m-tile 1: row 63
    assert np.array_equal(idx[3, 63], 63 * 32 + 24 + r8)       # the last eight weights of the first layer
    assert idx[3, 63, 7] == 2047
    assert np.array_equal(idx[4, 0], 2048 + np.array([0, 1, 2, 3, 8, 9, 10, 11]))       # neuron 0, k-group 0
    assert np.array_equal(idx[4, 16], 2048 + np.array([16, 17, 18, 19, 24, 25, 26, 27]))  # k-group 1
    assert np.array_equal(idx[4, 32], 2048 + np.array([4, 5, 6, 7, 12, 13, 14, 15]))    # k-group 2
    assert np.array_equal(idx[4, 15], 2048 + 15 * 64 + np.array([0, 1, 2, 3, 8, 9, 10, 11]))   # neuron 15
    assert np.array_equal(idx[5, 63], 2048 + 15 * 64 + 32 + np.array([20, 21, 22, 23, 28, 29, 30, 31]))   # neuron 15, k-step 1, k-group 3
    assert idx[5, 63, 7] == 3071
