"""numpy restatement of the density net's fragment image (include/nerficg_hip.h group 29; csrc/ngp_net.hip: density_frag_image_build).  Plain module: no test
functions.  Used by tests/test_density_frag_image_cpu.py and tests/test_gpu_density_frag_image.py.

The density weights are 3 072 fp16 values, row-major: the 64 x 32 first layer, then the 16 x 64 head.  The image is 6 slots x 64 lanes x 8 halves: slot f, lane l
holds the A fragment that the MFMA chain of the density net reads for that lane."""
import numpy as np

N_WEIGHTS = 64 * 32 + 16 * 64
N_SLOTS, N_LANES, N_ELEMS = 6, 64, 8


def image_indices() -> np.ndarray:
    """(6, 64, 8) int64: which of the 3 072 weights element e of lane l of slot f holds"""
    idx = np.empty((N_SLOTS, N_LANES, N_ELEMS), np.int64)
    lane = np.arange(N_LANES)[:, None]
    e = np.arange(N_ELEMS)[None, :]
    for f in range(4):   # first layer, 32x32x16 MFMA: m-tile f >> 1, k-step f & 1; lane = (row in the tile, half of the k-step)
        idx[f] = (32 * (f >> 1) + (lane & 31)) * 32 + 16 * (f & 1) + 8 * (lane >> 5) + e
    m, kg = lane & 15, lane >> 4
    for ks in range(2):  # 16-row head, 16x16x32 MFMA: k-step ks; lane = (neuron m, k-group kg), the k order of the layer in front folded in
        idx[4 + ks] = 2048 + 64 * m + 32 * ks + (e & 3) + 8 * (2 * (kg & 1) + (e >> 2)) + 4 * (kg >> 1)
    return idx


def image_of(weights: np.ndarray) -> np.ndarray:
    """weights: (3072,) of any dtype -> the (6, 64, 8) image of the same dtype"""
    weights = np.asarray(weights).reshape(-1)
    assert weights.size == N_WEIGHTS
    return weights[image_indices()]


def distinct_weights() -> np.ndarray:
    """3 072 fp16 values, all distinct and exact: (i - 1536) / 2048"""
    w = ((np.arange(N_WEIGHTS, dtype=np.float64) - 1536) / 2048).astype(np.float16)
    assert np.unique(w).size == N_WEIGHTS
    return w
