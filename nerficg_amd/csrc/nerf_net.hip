// nerf_net.hip -- the vanilla NeRF block (frequency encodings + n_layers x W MLP with skip re-entry + density head + feature layer + colour head),
// INFERENCE forward, as one kernel on v_mfma_f32_32x32x16_f16 (header group 17).  Reference: src/Methods/NeRF/Model.py:59-83, utils.py:12-36.
//
// ARITHMETIC CONTRACT (restated in f64 by tests/nerf_mlp_ref.py; DESIGN.md "NeRF block")
//   * weights and every MFMA operand (encoded inputs, hidden activations, feature-layer output) are fp16, converted round-to-nearest-even;
//     a weight beyond +-65504 is stored as +-65504.
//   * accumulation is f32 and STARTS at the f32 bias: z = bias + sum_k w_k h_k, k in the order of the matrix instruction.
//   * the next operand is  sat(relu(fp16(z))) : conversion FIRST (RNE, may give inf), THEN ReLU, THEN saturation to +-65504 -- the last two as
//     packed fp16 max / min.  The feature layer has no ReLU: sat(fp16(z)).  Since rounding is monotone and keeps 0 this equals fp16(clamp(relu(z))).
//   * sigma = relu(z) and rgb = 1 / (1 + expf(-z)) leave the f32 accumulator directly (accurate expf and division: no fast-math in this build).
//   * encodings: the argument a = x * 2^k is exact in f32 (a multiplication by a power of two).  sin / cos: nerf_sincos (nerf_net.h) -- n = rint(a 2/pi),
//     r = a - n pi/2 in three fused multiply-adds with pi/2 = C1 + C2 + C3 (C1 8 bits, C2 11 bits: n C1 and n C2 are exact for |n| < 2^12, the first
//     step is exact, the other two round once each at <= 2^-25), then the degree-7 / degree-8 minimax polynomials of Cephes sinf / cosf on
//     [-pi/4, pi/4] and the quadrant by n & 3.  |f32 value - f64 function| <= NRC_NERF_E_ENC = 2^-22 (2.4e-7) for |x| <= 8, k <= 9 (|a| <= 4096):
//     two reduction roundings (6e-8), the polynomials' approximation error and four evaluation roundings at values <= 1 (1.2e-7 together); a dense
//     scan of the same f32 sequence (tests/nerf_mlp_ref.py: sincos_model) finds 9.3e-8.  Every step is an explicit fmaf or a single product: the
//     compiler has nothing to contract.  Beyond |a| = 4096 the error grows with |n| (no longer a stated bound).  The appended raw input and every
//     sin / cos value are then rounded to fp16.
//   * each output row depends on its own input row and the weights only: a sample lives on one lane column of the matrix instruction, the k order is
//     fixed by the blob, and nothing is reduced across rows.
//
// FORMULATION.  H^T = W . X^T as in ngp_net.h: the weights are the A operand, the 32 samples of a wave the columns of B, and the f32 result tile
// converts in registers into the next layer's B fragments ("ACC order" of the k index, folded into the packed weights).  A workgroup is four waves =
// NRC_NERF_TILE_ROWS = 128 rows; all four walk the same sequence of weight "parts" in lockstep and share every part through LDS: the blob stores a
// part as [k-step][m-tile][lane] x 16 bytes, i.e. exactly the A fragments in the order they are consumed, so staging is a linear 16-byte copy and a
// fragment read is one conflict-free ds_read_b128 per MFMA.  Slabs of <= 32 KB are double-buffered: while slab i feeds the MFMAs, slab i + 1 (or the
// first slab of the NEXT part) travels L2 -> registers -> the other buffer; one barrier per slab.
#include "nerf_net.h"

namespace {

// Parameter list order: [initial_layers[0..L-1], density_layer, feature_layer, colour linears 0..n_color_layers-1, rgb linear] x (weight, bias).
void make_layout(const NerfCfg& c, NerfLayout& L) {
    const int W = c.width, NM = W / 32, np = enc_width(c.n_freq_pos, c.append_input), nd = enc_width(c.n_freq_dir, c.append_input);
    int n = 0, nl = 0;
    uint32_t off = 0, boff = 0;
    auto part = [&](int nmt, int nks, int src, int natural, int rows, int ld, int col_off, int kvalid) {
        L.part[n++] = make_part(off, nmt, nks, src, natural, rows, ld, col_off, kvalid);
    };
    auto linear = [&](int rows, int nmt, int src) { L.lin[nl++] = NerfLinear{boff, rows, nmt, src}; boff += (uint32_t)(nmt * 32); };
    int lin = 0;
    part(NM, 4, 2 * lin, 1, W, np, 0, np); linear(W, NM, 2 * lin + 1); lin++;
    for (int l = 1; l < c.n_layers; l++, lin++) {
        const int skip = (c.skip_mask >> l) & 1, ld = W + (skip ? np : 0);
        part(NM, W / 16, 2 * lin, 0, W, ld, 0, W);
        if (skip) part(NM, 4, 2 * lin, 1, W, ld, W, np);
        linear(W, NM, 2 * lin + 1);
    }
    part(1, W / 16, 2 * lin, 0, 1, W, 0, W); linear(1, 1, 2 * lin + 1); lin++;                  // density
    part(NM, W / 16, 2 * lin, 0, W, W, 0, W); linear(W, NM, 2 * lin + 1); lin++;                // feature
    part(NM / 2, W / 16, 2 * lin, 0, W / 2, W + nd, 0, W);                                      // colour 0: features ...
    part(NM / 2, 2, 2 * lin, 1, W / 2, W + nd, W, nd); linear(W / 2, NM / 2, 2 * lin + 1); lin++;   // ... and encoded direction BEHIND them
    for (int q = 1; q < c.n_color_layers; q++, lin++) { part(NM / 2, W / 32, 2 * lin, 0, W / 2, W / 2, 0, W / 2); linear(W / 2, NM / 2, 2 * lin + 1); }
    part(1, W / 32, 2 * lin, 0, 3, W / 2, 0, W / 2); linear(3, 1, 2 * lin + 1); lin++;
    close_layout(L, n, nl, off, boff);   // boff <= NRC_NERF_MAX_BIAS for every supported shape (a multiple of 32)
}

__global__ void __launch_bounds__(256) k_nerf_pack(NerfParams P, NerfLayout L, uint4* __restrict__ blob) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx < L.w_total) {
        int p = 0;
        while (p + 1 < L.n_parts && idx >= L.part[p + 1].off) p++;
        const NerfPart q = L.part[p];
        const uint32_t local = idx - q.off;
        const int lane = (int)(local & 63u), t = (int)(local >> 6), mt = t % q.nmt, s = t / q.nmt;
        const int row = 32 * mt + (lane & 31), hh = lane >> 5;
        const float* src = P.p[q.src];
        h8 f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = q.natural ? 16 * s + 8 * hh + j : 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3);
            f[j] = (row < q.rows && k < q.kvalid) ? to_h_sat(src[(size_t)row * q.ld + q.col_off + k]) : (_Float16)0.f;
        }
        blob[idx] = *reinterpret_cast<const uint4*>(&f);
    } else if (idx - L.w_total < L.b_total) {
        const uint32_t b = idx - L.w_total;
        int li = 0;
        while (li + 1 < L.n_linears && b >= L.lin[li + 1].off) li++;
        const NerfLinear q = L.lin[li];
        const int local = (int)(b - q.off), mt = local >> 5, hh = (local >> 4) & 1, i = local & 15;
        const int neuron = 32 * mt + (i & 3) + 8 * (i >> 2) + 4 * hh;
        reinterpret_cast<float*>(blob + L.w_total)[b] = neuron < q.rows ? P.p[q.src][neuron] : 0.f;
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <int NMT>
__device__ __forceinline__ void load_bias(f16v (&acc)[NMT], const float* bias, int hh) {
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) {
        const float4* b = reinterpret_cast<const float4*>(bias + (mt * 2 + hh) * 16);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 v = b[q];
            acc[mt][4 * q] = v.x; acc[mt][4 * q + 1] = v.y; acc[mt][4 * q + 2] = v.z; acc[mt][4 * q + 3] = v.w;
        }
    }
}

// frequency encoding of (x0, x1, x2) as NKS NATURAL-order fragments: element j of lane half hh of k-step s = feature 16 s + 8 hh + j of
// [x, then per dimension: cos(x 2^k) k < K, sin(x 2^k) k < K]; features >= the width are 0
template <int NKS>
__device__ __forceinline__ void encode_freq(float x0, float x1, float x2, int K, int append, int hh, h8* E) {
    const int width = 6 * K + (append ? 3 : 0);
#pragma unroll
    for (int s = 0; s < NKS; s++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int f = 16 * s + 8 * hh + j;
            float v = 0.f;
            if (f < width) {
                const int g = f - (append ? 3 : 0);
                if (g < 0) {
                    v = f == 0 ? x0 : (f == 1 ? x1 : x2);
                } else {
                    const int d = (g >= 2 * K) + (g >= 4 * K), rem = g - 2 * K * d, is_sin = rem >= K, k = rem - (is_sin ? K : 0);
                    const float x = d == 0 ? x0 : (d == 1 ? x1 : x2);
                    const float arg = x * __uint_as_float((uint32_t)(127 + k) << 23);   // exact: a power of two
                    float sn, cs;
                    nerf_sincos(arg, sn, cs);
                    v = is_sin ? sn : cs;
                }
            }
            E[s][j] = to_h_sat(v);
        }
}

// taps (test instantiation only): the fp16 operand of one stage, unpadded, row-major (M, width)
template <int NFR>
__device__ __forceinline__ void tap_natural(const h8* E, int width, _Float16* out, int64_t i, int hh) {
#pragma unroll
    for (int s = 0; s < NFR; s++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int f = 16 * s + 8 * hh + j;
            if (f < width) out[i * width + f] = E[s][j];
        }
}
template <int NFR>
__device__ __forceinline__ void tap_acc(const h8* H, int width, _Float16* out, int64_t i, int hh) {
#pragma unroll
    for (int s = 0; s < NFR; s++)
#pragma unroll
        for (int j = 0; j < 8; j++) out[i * width + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)] = H[s][j];
}

// training (TAP == 2): every stage's operand as the fragments the lanes hold, padded rows included, into the workspace behind tap_out (NerfWs)
template <int N>
__device__ __forceinline__ void save_stage(const h8* F, uint4* ws, const NerfWs& S, int t, int64_t tile32, int lane) {
    uint4* dst = ws + S.stage_base(S.saved_ks(t)) + tile32 * N * 64 + lane;
#pragma unroll
    for (int s = 0; s < N; s++) dst[s * 64] = *reinterpret_cast<const uint4*>(&F[s]);
}

// TAP: 0 = inference, 1 = one stage to tap_out (tests), 2 = training: every stage into the workspace
template <int W, int TAP>
__global__ void __launch_bounds__(256) k_nerf_forward(const float* __restrict__ positions, const float* __restrict__ directions, int64_t dir_group, int64_t M,
                                                      const uint4* __restrict__ blob, NerfCfg c, NerfLayout L, float* __restrict__ sigma,
                                                      float* __restrict__ rgb, int tap, _Float16* __restrict__ tap_out) {
    constexpr int NM = W / 32, NK = W / 16;
    __shared__ uint4 lds[2 * NRC_NERF_SLAB];
    __shared__ float4 bias_lds[NRC_NERF_MAX_BIAS / 4];   // every bias of the network, once per workgroup: a layer then starts with LDS reads, not an L2 round trip
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int64_t i = (int64_t)blockIdx.x * NRC_NERF_TILE_ROWS + (tid >> 6) * 32 + r;
    const bool valid = i < M;
    const int64_t ic = valid ? i : M - 1;
    for (uint32_t e = (uint32_t)tid; e < L.b_total / 4; e += 256u) bias_lds[e] = reinterpret_cast<const float4*>(blob + L.w_total)[e];
    const float* bias = reinterpret_cast<const float*>(bias_lds);

    Stream st{blob, lds, 0, 0};
#pragma unroll
    for (int q = 0; q < NRC_NERF_PF; q++) {
        const uint32_t e = (uint32_t)tid + 256u * q;
        if (e < L.part[0].first) lds[e] = blob[e];
    }

    h8 EP[4], ED[2];
    {
        const float* xp = positions + 3 * ic;
        encode_freq<4>(xp[0], xp[1], xp[2], c.n_freq_pos, c.append_input, hh, EP);
        const float* dp = directions + 3 * (ic / dir_group);
        encode_freq<2>(dp[0], dp[1], dp[2], c.n_freq_dir, c.append_input, hh, ED);
    }
    const int n_pos = 6 * c.n_freq_pos + (c.append_input ? 3 : 0), n_dir = 6 * c.n_freq_dir + (c.append_input ? 3 : 0);
    [[maybe_unused]] NerfWs S{(int64_t)gridDim.x * (NRC_NERF_TILE_ROWS / 32), NK, c.n_layers};
    [[maybe_unused]] uint4* ws = reinterpret_cast<uint4*>(tap_out);
    [[maybe_unused]] const int64_t tile32 = (int64_t)blockIdx.x * (NRC_NERF_TILE_ROWS / 32) + (tid >> 6);
    if constexpr (TAP == 2) { save_stage<4>(EP, ws, S, 0, tile32, lane); save_stage<2>(ED, ws, S, 1, tile32, lane); }
    if constexpr (TAP == 1) {
        if (valid && tap == 1) tap_natural<4>(EP, n_pos, tap_out, i, hh);
        if (valid && tap == 2) tap_natural<2>(ED, n_dir, tap_out, i, hh);
    }
    __syncthreads();

    f16v acc[NM];
    h8 H[NK];
    int li = 0;
    load_bias<NM>(acc, bias + L.lin[li++].off, hh);
    gemm_part<NM, 4>(acc, EP, L, st, tid, lane);
    to_operands<NM, true>(acc, H);
    if constexpr (TAP == 1) if (valid && tap == 3) tap_acc<NK>(H, W, tap_out, i, hh);
    if constexpr (TAP == 2) save_stage<NK>(H, ws, S, 2, tile32, lane);
    for (int l = 1; l < c.n_layers; l++) {
        load_bias<NM>(acc, bias + L.lin[li++].off, hh);
        gemm_part<NM, NK>(acc, H, L, st, tid, lane);
        if ((c.skip_mask >> l) & 1) gemm_part<NM, 4>(acc, EP, L, st, tid, lane);
        to_operands<NM, true>(acc, H);
        if constexpr (TAP == 1) if (valid && tap == 3 + l) tap_acc<NK>(H, W, tap_out, i, hh);
        if constexpr (TAP == 2) save_stage<NK>(H, ws, S, 2 + l, tile32, lane);
    }
    {   // density head: row 0 of a one-tile part
        f16v a1[1];
        load_bias<1>(a1, bias + L.lin[li++].off, hh);
        gemm_part<1, NK>(a1, H, L, st, tid, lane);
        if (valid && hh == 0) sigma[i] = fmaxf(a1[0][0], 0.f);
    }
    load_bias<NM>(acc, bias + L.lin[li++].off, hh);
    gemm_part<NM, NK>(acc, H, L, st, tid, lane);
    to_operands<NM, false>(acc, H);
    int t = 3 + c.n_layers;
    if constexpr (TAP == 1) if (valid && tap == t) tap_acc<NK>(H, W, tap_out, i, hh);
    if constexpr (TAP == 2) save_stage<NK>(H, ws, S, c.n_layers + 2, tile32, lane);
    // colour head: [features, encoded direction] -> W/2, then (n_color_layers - 1) x W/2 -> W/2, then 3
    f16v ac[NM / 2];
    h8 C[NK / 2];
    load_bias<NM / 2>(ac, bias + L.lin[li++].off, hh);
    gemm_part<NM / 2, NK>(ac, H, L, st, tid, lane);
    gemm_part<NM / 2, 2>(ac, ED, L, st, tid, lane);
    to_operands<NM / 2, true>(ac, C);
    t++;
    if constexpr (TAP == 1) if (valid && tap == t) tap_acc<NK / 2>(C, W / 2, tap_out, i, hh);
    if constexpr (TAP == 2) save_stage<NK / 2>(C, ws, S, c.n_layers + 3, tile32, lane);
    for (int q = 1; q < c.n_color_layers; q++) {
        load_bias<NM / 2>(ac, bias + L.lin[li++].off, hh);
        gemm_part<NM / 2, NK / 2>(ac, C, L, st, tid, lane);
        to_operands<NM / 2, true>(ac, C);
        t++;
        if constexpr (TAP == 1) if (valid && tap == t) tap_acc<NK / 2>(C, W / 2, tap_out, i, hh);
    }
    {
        f16v a1[1];
        load_bias<1>(a1, bias + L.lin[li++].off, hh);
        gemm_part<1, NK / 2>(a1, C, L, st, tid, lane);
        if (valid && hh == 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) rgb[3 * i + ch] = 1.f / (1.f + expf(-a1[0][ch]));
        }
    }
}

}  // namespace

extern "C" {

int nrc_nerf_supported(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                       int32_t append_input, int32_t skip_mask) {
    return cfg_supported(NerfCfg{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask}) ? 1 : 0;
}

int nrc_nerf_tile_rows(void) { return NRC_NERF_TILE_ROWS; }

int64_t nrc_nerf_packed_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                              int32_t append_input, int32_t skip_mask) {
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    NerfLayout L;
    make_layout(c, L);
    return (int64_t)L.w_total * 16 + (int64_t)L.b_total * 4;
}

int nrc_nerf_pack_weights(const float* const* params, int32_t n_params, int32_t width, int32_t n_layers, int32_t n_color_layers,
                          int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, void* blob,
                          nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (!params || !blob || (reinterpret_cast<uintptr_t>(blob) & 15u)) return NRC_ERR_INVALID;
    NerfLayout L;
    make_layout(c, L);
    if (n_params != 2 * L.n_linears) return NRC_ERR_INVALID;
    NerfParams P;
    for (int k = 0; k < 2 * NRC_NERF_MAX_LINEARS; k++) {
        P.p[k] = k < n_params ? params[k] : nullptr;
        if (k < n_params && !P.p[k]) return NRC_ERR_INVALID;
    }
    NRC_STAGE((hipStream_t)stream, nullptr);
    const uint32_t n = L.w_total + L.b_total;
    hipLaunchKernelGGL(k_nerf_pack, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, P, L, (uint4*)blob);
    NRC_LAUNCH_CHECK();
    NRC_STAGE((hipStream_t)stream, "k_nerf_pack");
    return NRC_OK;
}

int nrc_nerf_block_forward(const float* positions, const float* directions, int64_t dir_group, int64_t M, const void* blob, int32_t width,
                           int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                           int32_t append_input, int32_t skip_mask, float* sigma, float* rgb, int32_t tap, void* tap_out, nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (M < 0 || dir_group < 1 || tap < 0 || tap > 3 + n_layers + n_color_layers || (tap > 0 && !tap_out && M > 0)) return NRC_ERR_INVALID;
    if (M == 0) return NRC_OK;
    if (!positions || !directions || !blob || !sigma || !rgb || (reinterpret_cast<uintptr_t>(blob) & 15u)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(M, NRC_NERF_TILE_ROWS);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    NerfLayout L;
    make_layout(c, L);
    NRC_STAGE((hipStream_t)stream, nullptr);
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    _Float16* to = (_Float16*)tap_out;
    if (width == 256) {
        if (tap) hipLaunchKernelGGL((k_nerf_forward<256, 1>), grid, block, 0, s, positions, directions, dir_group, M, (const uint4*)blob, c, L, sigma, rgb, (int)tap, to);
        else hipLaunchKernelGGL((k_nerf_forward<256, 0>), grid, block, 0, s, positions, directions, dir_group, M, (const uint4*)blob, c, L, sigma, rgb, 0, to);
    } else {
        if (tap) hipLaunchKernelGGL((k_nerf_forward<128, 1>), grid, block, 0, s, positions, directions, dir_group, M, (const uint4*)blob, c, L, sigma, rgb, (int)tap, to);
        else hipLaunchKernelGGL((k_nerf_forward<128, 0>), grid, block, 0, s, positions, directions, dir_group, M, (const uint4*)blob, c, L, sigma, rgb, 0, to);
    }
    NRC_LAUNCH_CHECK();
    NRC_STAGE((hipStream_t)stream, "k_nerf_forward");
    return NRC_OK;
}

int nrc_nerf_train_supported(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                             int32_t append_input, int32_t skip_mask) {
    return train_cfg_supported(NerfCfg{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask}) ? 1 : 0;
}

int nrc_nerf_block_forward_train(const float* positions, const float* directions, int64_t dir_group, int64_t M, const void* blob, int32_t width,
                                 int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                                 int32_t append_input, int32_t skip_mask, float* sigma, float* rgb, void* workspace, nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (M < 0 || dir_group < 1) return NRC_ERR_INVALID;
    if (M == 0) return NRC_OK;
    if (!positions || !directions || !blob || !sigma || !rgb || !workspace || (reinterpret_cast<uintptr_t>(blob) & 15u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(M, NRC_NERF_TILE_ROWS);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    NerfLayout L;
    make_layout(c, L);
    NRC_STAGE((hipStream_t)stream, nullptr);
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    _Float16* ws = (_Float16*)workspace;
    if (width == 256) hipLaunchKernelGGL((k_nerf_forward<256, 2>), grid, block, 0, s, positions, directions, dir_group, M, (const uint4*)blob, c, L, sigma, rgb, 0, ws);
    else hipLaunchKernelGGL((k_nerf_forward<128, 2>), grid, block, 0, s, positions, directions, dir_group, M, (const uint4*)blob, c, L, sigma, rgb, 0, ws);
    NRC_LAUNCH_CHECK();
    NRC_STAGE((hipStream_t)stream, "k_nerf_forward_train");
    return NRC_OK;
}

}  // extern "C"
