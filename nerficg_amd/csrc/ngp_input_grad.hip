// ngp_input_grad.hip -- derivatives of the two input encodings with respect to their INPUT (include/nerficg_hip.h, group 3): what
// NetworkWithInputEncoding.backward hands back for `x` behind nrc_nwie_backward's d_in.
//
//   k_grid_input_grad<F, PAIR_MAJOR>   d(encoded features)/d(x01) of the multiresolution hash grid, contracted with d_in
//   k_sh_identity_input_grad           d(SH degree 4)/d(d01) contracted with d_in[0:16], and the identity columns d_in[16:32]
//
// Both are the derivative of what the forward pass computed in f32 BEFORE its final fp16 rounding of the feature (as tiny-cuda-nn does), and the
// grid's is the piecewise derivative of the cell the forward pass used: cell and fractions are grid_cell's, fmaf(scale, x, 0.5) and its floor.
// This translation unit is built without FMA contraction (nerficg_amd/build.py): the f32 sequence written here is the one that
// tests/input_grad_ref.py counts rounding by rounding.
#include "ngp_net.h"

#include <math.h>

namespace {

// GridCfg of a grid: validation, level offsets and sizes are nrc_grid_layout's (ngp_net.hip keeps its builder to itself); scale and resolution are
// restated from the same two expressions, and a level is hashed when its entries are fewer than res^3 (the dense stride no longer fits).
int input_grad_grid_cfg(int n_levels, int log2_T, int base_res, float pls, GridCfg& g) {
    uint32_t off[NRC_MAX_LEVELS + 1];
    if (n_levels > NRC_MAX_LEVELS) return NRC_ERR_INVALID;
    const int rc = nrc_grid_layout(n_levels, log2_T, base_res, pls, off);
    if (rc != NRC_OK) return rc;
    const float log2_pls = log2f(pls);
    for (int l = 0; l < NRC_MAX_LEVELS; l++) { g.offset[l] = 0; g.size[l] = 8; g.res[l] = 2; g.hashed[l] = 0; g.scale[l] = 1.f; }
    for (int l = 0; l < n_levels; l++) {
        const float scale = exp2f(l * log2_pls) * base_res - 1.0f;
        const uint32_t res = (uint32_t)ceilf(scale) + 1;
        const uint32_t n = off[l + 1] - off[l];
        g.offset[l] = off[l]; g.size[l] = n; g.res[l] = res; g.scale[l] = scale;
        g.hashed[l] = (uint64_t)n < (uint64_t)res * res * res ? 1u : 0u;
    }
    g.total_entries = off[n_levels];
    return NRC_OK;
}

// With s_k = sum_f g_f v_k[f] for the eight corners of the cell (Corner8 order: corner k is x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2)) the
// trilinear interpolant's derivative is
//   d/dx = scale [(1-wy)(1-wz)(s1-s0) + wy(1-wz)(s3-s2) + (1-wy)wz(s5-s4) + wy wz(s7-s6)]        and likewise for y (pairs k, k+2) and z (k, k+4).
// 256 threads = 64 consecutive samples x 4 waves; wave w owns the levels [n_levels w / 4, n_levels (w + 1) / 4): the level is wave-uniform, the index
// form a scalar branch.  The four partial sums meet in LDS and are added in wave order -- no atomics, no pre-zeroed output, the same bits every
// time.  A level whose upstream gradient is zero for a sample is skipped by that lane (no gathers): a row of zeros gathers nothing and gives 0.
// Every table read goes through the bounded descriptor (and grid_corners_u wraps / masks the index into its level): no position, NaN included,
// reads outside the table.
#define IG_LD 75   // floats between two components of a wave's partials: 11 c + sample is a different LDS bank for each of a half-wave's 32 (sample, c)
template <int F, bool PAIR_MAJOR>
__global__ void __launch_bounds__(256) k_grid_input_grad(const float* __restrict__ x, int64_t M, const float* __restrict__ d_feat,
                                                         const void* __restrict__ table, GridCfg g, int n_levels, float* __restrict__ d_x) {
    __shared__ float part[4][3][IG_LD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool live = i < M;
    const __amdgpu_buffer_rsrc_t trs = make_table_rsrc(table, g.total_entries * (uint32_t)(2 * F));
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = x[3 * i]; py = x[3 * i + 1]; pz = x[3 * i + 2]; }
    float ax = 0.f, ay = 0.f, az = 0.f;
    const int lvl_begin = n_levels * wave / 4, lvl_end = n_levels * (wave + 1) / 4;
#pragma unroll 1
    for (int level = lvl_begin; level < lvl_end; level++) {
        float gl[F];
        bool any = false;
        if (live) {
            if constexpr (PAIR_MAJOR) {   // [n_levels][M][2]
                const float2 v = *reinterpret_cast<const float2*>(d_feat + ((int64_t)level * M + i) * 2);
                gl[0] = v.x; gl[1] = v.y;
            } else if constexpr (F == 2) {
                const float2 v = *reinterpret_cast<const float2*>(d_feat + i * 32 + level * 2);
                gl[0] = v.x; gl[1] = v.y;
            } else {
                const float4 v = *reinterpret_cast<const float4*>(d_feat + i * 32 + level * 4);
                gl[0] = v.x; gl[1] = v.y; gl[2] = v.z; gl[3] = v.w;
            }
#pragma unroll
            for (int f = 0; f < F; f++) any = any || gl[f] != 0.f;
        }
        if (!any) continue;
        const float scale = g.scale[level];
        Corner8 c;
        if (g.hashed[level]) grid_corners_u<true>(px, py, pz, scale, g.res[level], g.size[level], g.offset[level], c);
        else grid_corners_u<false>(px, py, pz, scale, g.res[level], g.size[level], g.offset[level], c);
        float s[8];
        if constexpr (F == 2) {
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = __builtin_amdgcn_raw_buffer_load_b32(trs, c.e[k] << 2, 0, 0);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const h2 t = *reinterpret_cast<const h2*>(&v[k]);
                s[k] = fmaf(gl[1], (float)t[1], gl[0] * (float)t[0]);
            }
        } else {
            uint2 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const auto r = __builtin_amdgcn_raw_buffer_load_b64(trs, c.e[k] << 3, 0, 0);
                v[k] = make_uint2(r[0], r[1]);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const h4 t = *reinterpret_cast<const h4*>(&v[k]);
                s[k] = fmaf(gl[3], (float)t[3], fmaf(gl[2], (float)t[2], fmaf(gl[1], (float)t[1], gl[0] * (float)t[0])));
            }
        }
        // the fractions of grid_cell, by grid_cell's own expressions
        const float fx = fmaf(scale, px, 0.5f), fy = fmaf(scale, py, 0.5f), fz = fmaf(scale, pz, 0.5f);
        const float wx1 = fx - floorf(fx), wy1 = fy - floorf(fy), wz1 = fz - floorf(fz);
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1, wz0 = 1.f - wz1;
        const float dx = ((wy0 * wz0) * (s[1] - s[0]) + (wy1 * wz0) * (s[3] - s[2])) + ((wy0 * wz1) * (s[5] - s[4]) + (wy1 * wz1) * (s[7] - s[6]));
        const float dy = ((wx0 * wz0) * (s[2] - s[0]) + (wx1 * wz0) * (s[3] - s[1])) + ((wx0 * wz1) * (s[6] - s[4]) + (wx1 * wz1) * (s[7] - s[5]));
        const float dz = ((wx0 * wy0) * (s[4] - s[0]) + (wx1 * wy0) * (s[5] - s[1])) + ((wx0 * wy1) * (s[6] - s[2]) + (wx1 * wy1) * (s[7] - s[3]));
        ax += scale * dx;
        ay += scale * dy;
        az += scale * dz;
    }
    part[wave][0][lane] = ax;
    part[wave][1][lane] = ay;
    part[wave][2][lane] = az;
    __syncthreads();
    // the workgroup's 64 x 3 results are contiguous in d_x: thread t < 192 adds the four partials of element t in wave order and stores it
    const int t = threadIdx.x;
    if (t < 192) {
        const int sample = t / 3, comp = t - 3 * sample;
        const int64_t row = (int64_t)blockIdx.x * 64 + sample;
        if (row < M) d_x[row * 3 + comp] = ((part[0][comp][sample] + part[1][comp][sample]) + part[2][comp][sample]) + part[3][comp][sample];
    }
}

// One thread per sample.  input row: [d01 (3) | identity (16)] fp16, the row the forward pass read (encode_sh_id): d = 2 d01 - 1, and the 16
// polynomials of sh4_eval differentiated by hand.  d_in: (M, 32) f32, columns 0-15 the SH coefficients, 16-31 the identity dims.
// d_input: (M, 19) f32.  A configuration of degree < 4 has zero first-layer weights on the coefficients it lacks, hence zero d_in there.
__global__ void __launch_bounds__(256) k_sh_identity_input_grad(const __half* __restrict__ in, int ld, int64_t M, const float* __restrict__ d_in,
                                                                float* __restrict__ d_input) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const _Float16* row = reinterpret_cast<const _Float16*>(in) + i * ld;
    const float x = (float)row[0] * 2.f - 1.f, y = (float)row[1] * 2.f - 1.f, z = (float)row[2] * 2.f - 1.f;
    float gq[32];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const float4 v = *reinterpret_cast<const float4*>(d_in + i * 32 + 4 * q);
        gq[4 * q] = v.x; gq[4 * q + 1] = v.y; gq[4 * q + 2] = v.z; gq[4 * q + 3] = v.w;
    }
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    const float c1 = 0.48860251190291987f, c2 = 1.0925484305920792f, c3 = 0.94617469575755997f, c4 = 0.54627421529603959f, c5 = 0.59004358992664352f,
                c6 = 2.8906114426405538f, c7 = 0.45704579946446572f, c8 = 0.3731763325901154f, c9 = 1.4453057213202769f;
    const float q5 = 1.0f - 5.0f * z2, q3 = 3.0f * y2 - 3.0f * x2;
    // coefficient 0 is a constant; each sum runs over the coefficients in ascending order
    float gx = gq[3] * -c1;
    gx += gq[4] * (c2 * y);
    gx += gq[7] * (-c2 * z);
    gx += gq[8] * ((2.0f * c4) * x);
    gx += gq[9] * ((-6.0f * c5) * xy);
    gx += gq[10] * (c6 * yz);
    gx += gq[13] * (c7 * q5);
    gx += gq[14] * ((2.0f * c9) * xz);
    gx += gq[15] * (c5 * q3);
    float gy = gq[1] * -c1;
    gy += gq[4] * (c2 * x);
    gy += gq[5] * (-c2 * z);
    gy += gq[8] * ((-2.0f * c4) * y);
    gy += gq[9] * (c5 * q3);
    gy += gq[10] * (c6 * xz);
    gy += gq[11] * (c7 * q5);
    gy += gq[14] * ((-2.0f * c9) * yz);
    gy += gq[15] * ((6.0f * c5) * xy);
    float gz = gq[2] * c1;
    gz += gq[5] * (-c2 * y);
    gz += gq[6] * ((2.0f * c3) * z);
    gz += gq[7] * (-c2 * x);
    gz += gq[10] * (c6 * xy);
    gz += gq[11] * ((-10.0f * c7) * yz);
    gz += gq[12] * (c8 * (15.0f * z2 - 3.0f));
    gz += gq[13] * ((-10.0f * c7) * xz);
    gz += gq[14] * (c9 * (x2 - y2));
    float* out = d_input + i * 19;
    out[0] = 2.f * gx;   // d(d)/d(d01) = 2
    out[1] = 2.f * gy;
    out[2] = 2.f * gz;
#pragma unroll
    for (int j = 0; j < 16; j++) out[3 + j] = gq[16 + j];
}

}  // namespace

extern "C" {

int nrc_grid_backward_input(const float* x01, int64_t M, const float* d_features, int32_t d_features_pair_major, const void* table_f16,
                            int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                            float* d_x01, nrc_stream_t stream) {
    NRC_ENTER();
    if (M < 0 || (n_features != 2 && n_features != 4) || n_levels < 1 || n_levels * n_features > 32) return NRC_ERR_INVALID;
    if (d_features_pair_major != 0 && d_features_pair_major != 1) return NRC_ERR_INVALID;
    if (d_features_pair_major && n_features != 2) return NRC_ERR_INVALID;   // the pair-major layout is [n_levels][M][2]
    GridCfg g;
    const int rc = input_grad_grid_cfg(n_levels, log2_hashmap_size, base_resolution, per_level_scale, g);
    if (rc != NRC_OK) return rc;
    if ((uint64_t)g.total_entries * (uint64_t)(2 * n_features) > 0xffffffffull) return NRC_ERR_INVALID;   // the descriptor counts bytes in 32 bits
    if (M == 0) return NRC_OK;
    if (!x01 || !d_features || !table_f16 || !d_x01) return NRC_ERR_INVALID;
    const dim3 grid((unsigned)nrc_cdiv(M, 64)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define NRC_IG(F, P) hipLaunchKernelGGL((k_grid_input_grad<F, P>), grid, block, 0, s, x01, M, d_features, table_f16, g, (int)n_levels, d_x01)
    if (n_features == 4) NRC_IG(4, false);
    else if (d_features_pair_major) NRC_IG(2, true);
    else NRC_IG(2, false);
#undef NRC_IG
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_sh_identity_backward_input(const void* input_f16, int32_t input_ld, int64_t M, const float* d_in, float* d_input, nrc_stream_t stream) {
    NRC_ENTER();
    if (M < 0 || input_ld < 19) return NRC_ERR_INVALID;
    if (M == 0) return NRC_OK;
    if (!input_f16 || !d_in || !d_input) return NRC_ERR_INVALID;
    hipLaunchKernelGGL(k_sh_identity_input_grad, dim3((unsigned)nrc_cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, (const __half*)input_f16,
                       (int)input_ld, M, d_in, d_input);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
