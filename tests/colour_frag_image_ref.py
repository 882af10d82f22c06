"""numpy restatement of the colour net's fragment image (include/nerficg_hip.h group 30; csrc/ngp_net.hip: colour_frag_image_build).  Plain module: no test
functions.  Used by tests/test_colour_frag_image_cpu.py, tests/test_gpu_colour_frag_image.py and tests/test_gpu_frame_full_encoder.py.

The colour weights are 7 168 fp16 values, row-major: the 64 x 32 first layer (k 0-15 the SH coefficients, k 16-31 the density features), the 64 x 64 second
layer, then the 16 x 64 head.  The image is 14 slots x 64 lanes x 8 halves: slot f, lane l holds the A fragment that the MFMA chain of the colour net reads
for that lane -- C0 x 4, C1 x 8 in accumulator order, CO x 2."""
import numpy as np

N_WEIGHTS = 64 * 32 + 64 * 64 + 16 * 64
N_SLOTS, N_LANES, N_ELEMS = 14, 64, 8
L1, HEAD = 64 * 32, 64 * 32 + 64 * 64   # first weight of the second layer, of the head


def image_indices() -> np.ndarray:
    """(14, 64, 8) int64: which of the 7 168 weights element e of lane l of slot f holds"""
    idx = np.empty((N_SLOTS, N_LANES, N_ELEMS), np.int64)
    lane = np.arange(N_LANES)[:, None]
    e = np.arange(N_ELEMS)[None, :]
    for f in range(4):    # first layer, 32x32x16 MFMA, natural order: m-tile f >> 1, k-step f & 1; lane = (row in the tile, half of the k-step)
        idx[f] = (32 * (f >> 1) + (lane & 31)) * 32 + 16 * (f & 1) + 8 * (lane >> 5) + e
    for g in range(8):    # second layer, accumulator order: m-tile g >> 2, k-step g & 3; a lane half holds k 4 hh .. + 3 and 8 + 4 hh .. + 3 of the step
        idx[4 + g] = L1 + (32 * (g >> 2) + (lane & 31)) * 64 + 16 * (g & 3) + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3)
    m, kg = lane & 15, lane >> 4
    for ks in range(2):   # 16-row head, 16x16x32 MFMA: k-step ks; lane = (neuron m, k-group kg), the k order of the layer in front folded in
        idx[12 + ks] = HEAD + 64 * m + 32 * ks + (e & 3) + 8 * (2 * (kg & 1) + (e >> 2)) + 4 * (kg >> 1)
    return idx


def image_of(weights: np.ndarray) -> np.ndarray:
    """weights: (7168,) of any dtype -> the (14, 64, 8) image of the same dtype"""
    weights = np.asarray(weights).reshape(-1)
    assert weights.size == N_WEIGHTS
    return weights[image_indices()]


def distinct_weights() -> np.ndarray:
    """7 168 fp16 values, all distinct: the bit patterns 0x3000 + i, normal halves from 0.125 up to 16 (an arithmetic sequence of 7 168 values would need 13
    significant bits, fp16 holds 11)"""
    w = (0x3000 + np.arange(N_WEIGHTS)).astype(np.uint16).view(np.float16).copy()
    assert np.unique(w).size == N_WEIGHTS and np.isfinite(w.astype(np.float32)).all()
    return w
