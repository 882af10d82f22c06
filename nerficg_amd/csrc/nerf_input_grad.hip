// nerf_input_grad.hip -- the vanilla NeRF block's gradient with respect to its INPUTS (header group 20): sample positions and viewing directions.  One
// kernel on v_mfma_f32_32x32x16_f16 that runs after the training backward of the same batch (nerf_grad.hip) and reads the fp16 pre-activation gradient
// stages that backward left in the workspace, plus a small fixed-order reduction when several rows share a direction.  The workspace layout (NerfWs), the
// streamed GEMM (gemm_part) and the forward's sin / cos routine (nerf_sincos) come from nerf_net.h.
//
// ARITHMETIC CONTRACT (restated in f64 by tests/nerf_input_grad_ref.py).  G[.] are the gradient stages of the backward, scaled by S = 2^e;
// W16 the fp16 weights (the same values as the two other blobs: round-to-nearest-even, clamped at +-65504); W = width, n_pos / n_dir the encoded widths.
//   * encoded-input gradients: fp16 operands, ONE f32 accumulator per output starting at 0, in the order of the matrix instruction over the parts in the
//     order given; no fp16 conversion, no saturation, no mask:
//       dE_pos[m, i] = sum_o W16_0[o, i] G[H_1][m, o] + sum_{k in skips, ascending} sum_o W16_k[o, W + i] G[H_k+1][m, o]
//       dE_dir[m, j] = sum_o W16_colour[o, W + j] G[C_1][m, o]
//   * scale: e is read from the workspace header on the device (what the backward's automatic scale left there), or is the caller's fixed power of two,
//     validated exactly as nrc_nerf_block_backward validates it.  No host synchronisation.
//   * encoding backward, f32, per row and input component c: a_k = x_c 2^k (exact), (s_k, c_k) = nerf_sincos(a_k) -- the forward's own routine --
//       dx_c = [append] dE[c] + sum_{k<K} 2^k (c_k dE[sin_c,k] - s_k dE[cos_c,k]),   columns as FrequencyEncoding lays them out: 3 append + 2 K c + k for
//     cos, + K for sin.  Every addend is one rounded product (c_k dE or s_k dE) times the exact 2^k.  SUMMATION ORDER: a row lives on two lanes (lane
//     halves hh = 0, 1 of the matrix instruction's result); each half adds the addends of the encoded columns it holds -- column f of a 32-column tile is
//     on half (f >> 2) & 1 -- in ascending column order into one f32 partial per component, starting at 0; then half 0 + half 1; then ONE multiplication
//     by 2^-e (exact unless the result is subnormal).
//   * d_positions (M, 3) is that value for the position.  For the direction the per-row value is written directly when dir_group = 1; otherwise it goes
//     to scratch and d_directions[g, c] is the sum over the rows of group g (the last group may be partial): lane l of one wave per group adds rows
//     l, l + 64, .. in ascending order starting at 0, then a 6-step xor butterfly (distances 32, 16, .. 1) over the lanes.  No floating-point atomics: two
//     calls give the same bits; a row's d_positions (and, with dir_group = 1, its d_directions) depend on that row and the weights only.
//   * padded rows write nothing.  d_enc_pos / d_enc_dir (tests): the f32 accumulators dE, still scaled by S.
#include <math.h>

#include "nerf_net.h"

namespace {

// ---- the input stream -----------------------------------------------------------------------------------------------------------------------------
// A[row = encoded feature i, NATURAL order][k = output o of the linear, ACC order of the gradient stage] = W16[o, col_off + i], in the order of use.
void make_layout_i(const NerfCfg& c, NerfLayout& L) {
    const int W = c.width, NK = W / 16, np = enc_width(c.n_freq_pos, c.append_input), nd = enc_width(c.n_freq_dir, c.append_input);
    const int Ln = c.n_layers;
    int n = 0;
    uint32_t off = 0;
    L.part[n++] = make_part(off, 2, NK, 0, 0, np, np, 0, W);                                                      // all of W_0: dE_pos <- G(H_1)
    for (int k = 1; k < Ln; k++)
        if ((c.skip_mask >> k) & 1) L.part[n++] = make_part(off, 2, NK, 2 * k, 0, np, W + np, W, W);               // skip columns: dE_pos <- G(H_k+1)
    L.part[n++] = make_part(off, 1, NK / 2, 2 * (Ln + 2), 0, nd, W + nd, W, W / 2);                                // direction columns: dE_dir <- G(C_1)
    close_layout(L, n, 0, off, 0);
}

__global__ void __launch_bounds__(256) k_nerf_pack_i(NerfParams P, NerfLayout L, uint4* __restrict__ blob) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= L.w_total) return;
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
        const int k = 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3);
        f[j] = (row < q.rows && k < q.kvalid) ? to_h_sat(src[(size_t)k * q.ld + q.col_off + row]) : (_Float16)0.f;
    }
    blob[idx] = *reinterpret_cast<const uint4*>(&f);
}

// ---- scale (the rule of nerf_grad.hip) -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int scale_exponent(const int32_t* hdr, int fixed, int fixed_exp) {
    if (fixed) return fixed_exp;
    const uint32_t bits = (uint32_t)hdr[0];
    if (bits == 0u || bits >= 0x7f800000u) return 0;
    const int ex = (int)(bits >> 23);
    const int fl = ex > 0 ? ex - 127 : (31 - __clz((int)bits)) - 149;
    const int e = 12 - fl;
    return e > 126 ? 126 : (e < -126 ? -126 : e);
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }   // -126 <= e <= 127

template <int N>
__device__ __forceinline__ void load_stage(h8* F, const uint4* ws, int64_t base, int64_t tile32, int lane) {
    const uint4* src = ws + base + tile32 * N * 64 + lane;
#pragma unroll
    for (int s = 0; s < N; s++) { const uint4 v = src[s * 64]; F[s] = *reinterpret_cast<const h8*>(&v); }
}

// encoded column held in register reg of m-tile mt on lane half hh
__device__ __forceinline__ int acc_col(int mt, int reg, int hh) { return 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// this lane half's share of dx: the addends of its columns, ascending, into one partial per component
template <int NMT>
__device__ __forceinline__ void encoding_backward(const f16v (&acc)[NMT], float x0, float x1, float x2, int K, int append, int hh, float (&g)[3]) {
    const int width = 6 * K + (append ? 3 : 0);
    g[0] = 0.f; g[1] = 0.f; g[2] = 0.f;
#pragma unroll
    for (int mt = 0; mt < NMT; mt++)
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int f = acc_col(mt, reg, hh);
            if (f < width) {
                const float v = acc[mt][reg];
                const int q = f - (append ? 3 : 0);
                int d;
                float term;
                if (q < 0) {
                    d = f;
                    term = v;
                } else {
                    d = (q >= 2 * K) + (q >= 4 * K);
                    const int rem = q - 2 * K * d, is_sin = rem >= K, k = rem - (is_sin ? K : 0);
                    const float x = d == 0 ? x0 : (d == 1 ? x1 : x2);
                    const float p2 = __uint_as_float((uint32_t)(127 + k) << 23);
                    float sn, cs;
                    nerf_sincos(__fmul_rn(x, p2), sn, cs);
                    term = __fmul_rn(p2, is_sin ? __fmul_rn(cs, v) : -__fmul_rn(sn, v));
                }
                if (d == 0) g[0] = __fadd_rn(g[0], term);
                else if (d == 1) g[1] = __fadd_rn(g[1], term);
                else g[2] = __fadd_rn(g[2], term);
            }
        }
}

template <int NMT>
__device__ __forceinline__ void write_enc(const f16v (&acc)[NMT], int width, float* __restrict__ out, int64_t i, int hh) {
#pragma unroll
    for (int mt = 0; mt < NMT; mt++)
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int f = acc_col(mt, reg, hh);
            if (f < width) out[i * width + f] = acc[mt][reg];
        }
}

template <int W>
__global__ void __launch_bounds__(256) k_nerf_input_grad(const float* __restrict__ positions, const float* __restrict__ directions, int64_t dir_group, int64_t M,
                                                         const uint4* __restrict__ blob_i, NerfCfg c, NerfLayout L, const uint4* ws, int fixed, int fixed_exp,
                                                         float* __restrict__ d_positions, float* d_dir_rows, float* __restrict__ d_enc_pos,
                                                         float* __restrict__ d_enc_dir) {
    constexpr int NK = W / 16;
    __shared__ uint4 lds[2 * NRC_NERF_SLAB];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int64_t i = (int64_t)blockIdx.x * NRC_NERF_TILE_ROWS + (tid >> 6) * 32 + r;
    const int64_t tile32 = (int64_t)blockIdx.x * (NRC_NERF_TILE_ROWS / 32) + (tid >> 6);
    const NerfWs S{(int64_t)gridDim.x * (NRC_NERF_TILE_ROWS / 32), NK, c.n_layers};
    const bool valid = i < M;
    const int64_t ic = valid ? i : M - 1;
    const float inv_scale = pow2f(-scale_exponent(reinterpret_cast<const int32_t*>(ws), fixed, fixed_exp));

    Stream st{blob_i, lds, 0, 0};
#pragma unroll
    for (int q = 0; q < NRC_NERF_PF; q++) {
        const uint32_t e = (uint32_t)tid + 256u * q;
        if (e < L.part[0].first) lds[e] = blob_i[e];
    }
    __syncthreads();

    f16v ap[2];
    ap[0] = zero16(); ap[1] = zero16();
    {
        h8 G[NK];
        load_stage<NK>(G, ws, S.stage_base(S.grad_ks(3 + c.n_layers)), tile32, lane);              // G(H_1) through all of W_0
        gemm_part<2, NK>(ap, G, L, st, tid, lane);
        for (int k = 1; k < c.n_layers; k++)
            if ((c.skip_mask >> k) & 1) {                                                            // G(H_k+1) through the skip columns of W_k
                load_stage<NK>(G, ws, S.stage_base(S.grad_ks(3 + c.n_layers - k)), tile32, lane);
                gemm_part<2, NK>(ap, G, L, st, tid, lane);
            }
    }
    f16v ad[1];
    ad[0] = zero16();
    {
        h8 C[NK / 2];
        load_stage<NK / 2>(C, ws, S.stage_base(S.grad_ks(1)), tile32, lane);                        // G(C_1) through the direction columns
        gemm_part<1, NK / 2>(ad, C, L, st, tid, lane);
    }
    const int n_pos = 6 * c.n_freq_pos + (c.append_input ? 3 : 0), n_dir = 6 * c.n_freq_dir + (c.append_input ? 3 : 0);
    if (valid && d_enc_pos) write_enc<2>(ap, n_pos, d_enc_pos, i, hh);
    if (valid && d_enc_dir) write_enc<1>(ad, n_dir, d_enc_dir, i, hh);

    const float* xp = positions + 3 * ic;
    const float* dp = directions + 3 * (ic / dir_group);
    float gp[3], gd[3];
    encoding_backward<2>(ap, xp[0], xp[1], xp[2], c.n_freq_pos, c.append_input, hh, gp);
    encoding_backward<1>(ad, dp[0], dp[1], dp[2], c.n_freq_dir, c.append_input, hh, gd);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        gp[ch] = __fadd_rn(gp[ch], __shfl_xor(gp[ch], 32));
        gd[ch] = __fadd_rn(gd[ch], __shfl_xor(gd[ch], 32));
    }
    if (valid && hh == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            d_positions[3 * i + ch] = __fmul_rn(gp[ch], inv_scale);
            d_dir_rows[3 * i + ch] = __fmul_rn(gd[ch], inv_scale);
        }
    }
}

// one wave per group of dir_group rows: lane-strided partial sums in ascending row order, then the xor butterfly
__global__ void __launch_bounds__(256) k_nerf_dir_reduce(const float* __restrict__ rows, int64_t dir_group, int64_t M, int64_t n_groups, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const int64_t r0 = g * dir_group, r1 = r0 + dir_group < M ? r0 + dir_group : M;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int64_t row = r0 + lane; row < r1; row += 64) {
        a0 = __fadd_rn(a0, rows[3 * row]);
        a1 = __fadd_rn(a1, rows[3 * row + 1]);
        a2 = __fadd_rn(a2, rows[3 * row + 2]);
    }
    a0 = nrc_group_sum<64>(a0);
    a1 = nrc_group_sum<64>(a1);
    a2 = nrc_group_sum<64>(a2);
    if (lane == 0) { out[3 * g] = a0; out[3 * g + 1] = a1; out[3 * g + 2] = a2; }
}

inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

}  // namespace

extern "C" {

int64_t nrc_nerf_packed_input_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                                    int32_t append_input, int32_t skip_mask) {
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    NerfLayout L;
    make_layout_i(c, L);
    return (int64_t)L.w_total * 16;
}

int nrc_nerf_pack_weights_input(const float* const* params, int32_t n_params, int32_t width, int32_t n_layers, int32_t n_color_layers,
                                int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, void* blob,
                                nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (!params || !blob || (reinterpret_cast<uintptr_t>(blob) & 15u)) return NRC_ERR_INVALID;
    if (n_params != 2 * (n_layers + 4)) return NRC_ERR_INVALID;
    NerfLayout L;
    make_layout_i(c, L);
    NerfParams P;
    for (int k = 0; k < 2 * NRC_NERF_MAX_LINEARS; k++) {
        P.p[k] = k < n_params ? params[k] : nullptr;
        if (k < n_params && !P.p[k]) return NRC_ERR_INVALID;
    }
    NRC_STAGE((hipStream_t)stream, nullptr);
    hipLaunchKernelGGL(k_nerf_pack_i, dim3((L.w_total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, P, L, (uint4*)blob);
    NRC_LAUNCH_CHECK();
    NRC_STAGE((hipStream_t)stream, "k_nerf_pack_i");
    return NRC_OK;
}

int nrc_nerf_block_input_grad(const float* positions, const float* directions, int64_t dir_group, int64_t M, const void* blob_input, int32_t width,
                              int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input,
                              int32_t skip_mask, void* workspace, float grad_scale, float* d_positions, float* d_directions, float* d_enc_pos, float* d_enc_dir,
                              nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    int fixed = 0, fixed_exp = 0;
    if (grad_scale != 0.f) {   // as nrc_nerf_block_backward: a positive power of two inside the range the kernels can invert
        if (!(grad_scale > 0.f) || frexpf(grad_scale, &fixed_exp) != 0.5f) return NRC_ERR_INVALID;
        fixed = 1;
        fixed_exp -= 1;
        if (fixed_exp < -126 || fixed_exp > 126) return NRC_ERR_INVALID;
    }
    if (M < 0 || dir_group < 1) return NRC_ERR_INVALID;
    if (M == 0) return NRC_OK;
    if (!positions || !directions || !blob_input || !workspace || !d_positions || !d_directions || (reinterpret_cast<uintptr_t>(blob_input) & 15u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u) || misaligned4(positions) || misaligned4(directions) || misaligned4(d_positions) ||
        misaligned4(d_directions) || misaligned4(d_enc_pos) || misaligned4(d_enc_dir)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(M, NRC_NERF_TILE_ROWS);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    const NerfWs S = make_ws(c, M);
    // the per-row direction gradients of a grouped call go where the weight gradient's partial sums were: the backward has consumed them
    float* scratch = reinterpret_cast<float*>((uint4*)workspace + S.partial_base());
    const int64_t scratch_bytes = nrc_nerf_train_workspace_bytes(width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input,
                                                                 skip_mask, M) - S.partial_base() * 16;
    const bool grouped = dir_group > 1;
    if (grouped && scratch_bytes < M * 12) return NRC_ERR_INVALID;
    const int64_t n_groups = nrc_cdiv(M, dir_group), rblocks = nrc_cdiv(n_groups, 4);
    if (rblocks > 0x7fffffff) return NRC_ERR_INVALID;
    NerfLayout L;
    make_layout_i(c, L);
    hipStream_t s = (hipStream_t)stream;
    float* rows = grouped ? scratch : d_directions;
    NRC_STAGE(s, nullptr);
    if (width == 256) hipLaunchKernelGGL((k_nerf_input_grad<256>), dim3((unsigned)blocks), dim3(256), 0, s, positions, directions, dir_group, M, (const uint4*)blob_input, c, L, (const uint4*)workspace, fixed, fixed_exp, d_positions, rows, d_enc_pos, d_enc_dir);
    else hipLaunchKernelGGL((k_nerf_input_grad<128>), dim3((unsigned)blocks), dim3(256), 0, s, positions, directions, dir_group, M, (const uint4*)blob_input, c, L, (const uint4*)workspace, fixed, fixed_exp, d_positions, rows, d_enc_pos, d_enc_dir);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_input_grad");
    if (grouped) {
        hipLaunchKernelGGL(k_nerf_dir_reduce, dim3((unsigned)rblocks), dim3(256), 0, s, (const float*)scratch, dir_group, M, n_groups, d_directions);
        NRC_LAUNCH_CHECK();
        NRC_STAGE(s, "k_nerf_dir_reduce");
    }
    return NRC_OK;
}

}  // extern "C"
