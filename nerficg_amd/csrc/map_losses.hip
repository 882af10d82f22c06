// map_losses.hip -- the regularisers on the 3DGS rasterizer's depth and alpha maps as three launches (include/nerficg_hip.h group 15):
// depth_smoothness_loss (src/Optim/Losses/DepthSmoothness.py:31-43), background_entropy (src/Optim/Losses/BackgroundEntropy.py:6-8) and the
// depth / (alpha + 1e-6) normalisation in front of them (InstantNGP/Renderer.py:82), ~30 tensor operations each way as the reference writes them.
//
//   d      = normalize ? depth / (alpha + 1e-6f) : depth
//   lap_x  = (d[x-1] + d[x+1]) - 2 d[x],  x in [1, W-2]        w_x = expf(-(sum_c |I_c[x] - I_c[x-1]|) / C)        S_x = mean |lap_x w_x|
//   (the same along y)                     a = clamp(alpha, 1e-6f, 1 - 1e-6f)      E = mean(-a logf(a) [- (1 - a) logf(1 - a)])
//   loss   = lambda_smooth (S_x + S_y) + lambda_entropy E
//
// FORWARD: k_map_fwd, one workgroup per 32 x 16 tile, stages d (one-pixel halo) and the image channels (left / upper neighbour) in LDS with row loads,
// every thread sums its two pixels' terms, the workgroup writes {sum_x, sum_y, sum_e, 0} -- no atomics.  k_map_reduce (one workgroup) adds the partial
// sums in a fixed order with double accumulators and writes loss4 = {loss, S_x, S_y, E}: the same input gives the same bits.
// BACKWARD: k_map_bwd, one stencil and a gather.  With k_x = g lambda_smooth / N_x and the per-centre coefficients
//   c_x = sign(lap_x) w_x k_x          a_x = |lap_x| w_x k_x / C                 (zero where x is no centre of the plane)
// a pixel collects   dL/dd = (c_x[x-1] + c_x[x+1]) - 2 c_x[x] + the same along y      (the Laplacian of the coefficient map: the 1, -2, 1 of the three terms)
//                    dL/dI_c = -a_x[x] sign(I_c[x] - I_c[x-1]) + a_x[x+1] sign(I_c[x+1] - I_c[x]) + the same along y
// so the coefficient maps are built once per tile with a one-pixel halo in LDS (from d with a two-pixel halo) and nothing is scattered.  sign(0) = 0.
// Through the normalisation: dL/ddepth = dL/dd / (alpha + 1e-6f), dL/dalpha = -(dL/dd d) / (alpha + 1e-6f) + the entropy term, which is zero outside the
// clamp and passes at the bounds (torch.clamp).  g = the upstream gradient of the loss value, a device scalar (NULL: 1).
// expf / logf / the divisions are the accurate ones (no fast-math; the translation unit is built with -ffp-contract=off, see build.py).
#include <math.h>

#include "common.h"

namespace {

constexpr int MT_X = 32, MT_Y = 16, MT_N = 256;   // tile and workgroup: 8 rows of 32 threads, two pixels (rows ty, ty + 8) per thread
constexpr float M_EPS = 1e-6f;
constexpr float M_LO = 1e-6f, M_HI = 1.0f - 1e-6f;

__device__ __forceinline__ float m_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// a RH x RW window of one plane with its origin at (y0, x0) into LDS, zero outside the plane; consecutive lanes read consecutive pixels of a row.
// NORM: the value is src / (alpha + 1e-6f)
template <int RH, int RW, int LP, bool NORM>
__device__ __forceinline__ void m_stage(float (*dst)[LP], const float* __restrict__ src, const float* __restrict__ alpha, int y0, int x0, int H, int W) {
    static_assert(RW <= LP, "row pitch");
    for (int k = threadIdx.x; k < RH * RW; k += MT_N) {
        const int r = k / RW, c = k - r * RW;
        const int y = y0 + r, x = x0 + c;
        float v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int o = y * W + x;
            v = src[o];
            if (NORM) v = v / (alpha[o] + M_EPS);
        }
        dst[r][c] = v;
    }
}

__global__ void __launch_bounds__(MT_N) k_map_fwd(const float* __restrict__ depth, const float* __restrict__ alpha, const float* __restrict__ image, int C, int H, int W,
                                                  int normalize, int smooth, int entropy, int symmetrical, float* __restrict__ partial) {
    __shared__ float sd[MT_Y + 2][MT_X + 3];          // d, origin (y0 - 1, x0 - 1)
    __shared__ float si[4][MT_Y + 1][MT_X + 1];       // image channels, origin (y0 - 1, x0 - 1): the left and the upper neighbour only
    __shared__ float red[3][MT_N / 64];
    const int x0 = blockIdx.x * MT_X, y0 = blockIdx.y * MT_Y;
    const size_t plane = (size_t)blockIdx.z * H * W;  // wave-uniform base, 32-bit offsets inside a plane
    if (smooth) {
        if (normalize) m_stage<MT_Y + 2, MT_X + 2, MT_X + 3, true>(sd, depth + plane, alpha + plane, y0 - 1, x0 - 1, H, W);
        else m_stage<MT_Y + 2, MT_X + 2, MT_X + 3, false>(sd, depth + plane, nullptr, y0 - 1, x0 - 1, H, W);
        for (int c = 0; c < C; c++) m_stage<MT_Y + 1, MT_X + 1, MT_X + 1, false>(si[c], image + (plane * C + (size_t)c * H * W), nullptr, y0 - 1, x0 - 1, H, W);
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = x0 + tx;
    const float fC = (float)C;
    float sx = 0.f, sy = 0.f, se = 0.f;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ly = ty + 8 * i, y = y0 + ly;
        if (x >= W || y >= H) continue;
        if (smooth) {
            const float mi2 = 2.f * sd[ly + 1][tx + 1];
            if (x >= 1 && x <= W - 2) {
                const float lap = (sd[ly + 1][tx] + sd[ly + 1][tx + 2]) - mi2;
                float m = 0.f;
                for (int c = 0; c < C; c++) m += fabsf(si[c][ly + 1][tx + 1] - si[c][ly + 1][tx]);
                sx += fabsf(lap * expf(-(m / fC)));
            }
            if (y >= 1 && y <= H - 2) {
                const float lap = (sd[ly][tx + 1] + sd[ly + 2][tx + 1]) - mi2;
                float m = 0.f;
                for (int c = 0; c < C; c++) m += fabsf(si[c][ly + 1][tx + 1] - si[c][ly][tx + 1]);
                sy += fabsf(lap * expf(-(m / fC)));
            }
        }
        if (entropy) {
            float a = alpha[plane + (size_t)(y * W + x)];
            a = a < M_LO ? M_LO : (a > M_HI ? M_HI : a);
            float e = -a * logf(a);
            if (symmetrical) { const float b = 1.f - a; e -= b * logf(b); }
            se += e;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sx += __shfl_xor(sx, d, 64); sy += __shfl_xor(sy, d, 64); se += __shfl_xor(se, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sx; red[1][threadIdx.x >> 6] = sy; red[2][threadIdx.x >> 6] = se; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        reinterpret_cast<float4*>(partial)[blk] = make_float4((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]),
                                                              (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]), 0.f);
    }
}

// the loss value from the workgroups' partial sums: one workgroup, double accumulators, a fixed order (k_photo_reduce of ssim.hip with three sums).
// out = {lambda_smooth (S_x + S_y) + lambda_entropy E, S_x, S_y, E}
__global__ void __launch_bounds__(1024) k_map_reduce(const float* __restrict__ partial, int64_t n_blocks, double inv_nx, double inv_ny, double inv_ne, float lambda_smooth,
                                                     float lambda_entropy, float* __restrict__ out) {
    __shared__ double red[3][16];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t k0 = threadIdx.x; k0 < n_blocks; k0 += 4 * 1024) {   // four independent loads per turn
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t k = k0 + (int64_t)u * 1024;
            v[u] = k < n_blocks ? reinterpret_cast<const float4*>(partial)[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { a += (double)v[u].x; b += (double)v[u].y; c += (double)v[u].z; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); c += __shfl_xor(c, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0, sc = 0.0;
        for (int w = 0; w < 16; w++) { sa += red[0][w]; sb += red[1][w]; sc += red[2][w]; }
        const double Sx = sa * inv_nx, Sy = sb * inv_ny, E = sc * inv_ne;
        double loss = 0.0;
        if (lambda_smooth != 0.f) loss += (double)lambda_smooth * (Sx + Sy);
        if (lambda_entropy != 0.f) loss += (double)lambda_entropy * E;
        out[0] = (float)loss; out[1] = (float)Sx; out[2] = (float)Sy; out[3] = (float)E;
    }
}

// kx = lambda_smooth / N_x, ky = lambda_smooth / N_y, ke = lambda_entropy / N_e; `smooth` / `entropy`: which terms take part; any of the three outputs may be NULL
__global__ void __launch_bounds__(MT_N) k_map_bwd(const float* __restrict__ depth, const float* __restrict__ alpha, const float* __restrict__ image, int C, int H, int W,
                                                  int normalize, int smooth, int entropy, int symmetrical, float kx, float ky, float ke, const float* __restrict__ upstream,
                                                  float* __restrict__ g_depth, float* __restrict__ g_alpha, float* __restrict__ g_image) {
    __shared__ float sd[MT_Y + 4][MT_X + 5];          // d, origin (y0 - 2, x0 - 2)
    __shared__ float si[4][MT_Y + 3][MT_X + 3];       // image channels, origin (y0 - 2, x0 - 2), up to (y0 + MT_Y, x0 + MT_X)
    __shared__ float cxs[MT_Y + 2][MT_X + 3], axs[MT_Y + 2][MT_X + 3], cys[MT_Y + 2][MT_X + 3], ays[MT_Y + 2][MT_X + 3];   // centres, origin (y0 - 1, x0 - 1)
    const int x0 = blockIdx.x * MT_X, y0 = blockIdx.y * MT_Y;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float g = upstream ? upstream[0] : 1.f;
    const float fC = (float)C;
    if (smooth) {
        if (normalize) m_stage<MT_Y + 4, MT_X + 4, MT_X + 5, true>(sd, depth + plane, alpha + plane, y0 - 2, x0 - 2, H, W);
        else m_stage<MT_Y + 4, MT_X + 4, MT_X + 5, false>(sd, depth + plane, nullptr, y0 - 2, x0 - 2, H, W);
        for (int c = 0; c < C; c++) m_stage<MT_Y + 3, MT_X + 3, MT_X + 3, false>(si[c], image + (plane * C + (size_t)c * H * W), nullptr, y0 - 2, x0 - 2, H, W);
        __syncthreads();
        const float gkx = g * kx, gky = g * ky;
        const float gkxc = gkx / fC, gkyc = gky / fC;
        for (int k = threadIdx.x; k < (MT_Y + 2) * (MT_X + 2); k += MT_N) {
            const int r = k / (MT_X + 2), c = k - r * (MT_X + 2);
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            const float mi2 = 2.f * sd[r + 1][c + 1];
            float cx = 0.f, ax = 0.f, cy = 0.f, ay = 0.f;
            if (y >= 0 && y < H && x >= 1 && x <= W - 2) {
                const float lap = (sd[r + 1][c] + sd[r + 1][c + 2]) - mi2;
                float m = 0.f;
                for (int ch = 0; ch < C; ch++) m += fabsf(si[ch][r + 1][c + 1] - si[ch][r + 1][c]);
                const float w = expf(-(m / fC));
                cx = m_sign(lap) * w * gkx;
                ax = fabsf(lap) * w * gkxc;
            }
            if (x >= 0 && x < W && y >= 1 && y <= H - 2) {
                const float lap = (sd[r][c + 1] + sd[r + 2][c + 1]) - mi2;
                float m = 0.f;
                for (int ch = 0; ch < C; ch++) m += fabsf(si[ch][r + 1][c + 1] - si[ch][r][c + 1]);
                const float w = expf(-(m / fC));
                cy = m_sign(lap) * w * gky;
                ay = fabsf(lap) * w * gkyc;
            }
            cxs[r][c] = cx; axs[r][c] = ax; cys[r][c] = cy; ays[r][c] = ay;
        }
        __syncthreads();
    }
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = x0 + tx;
    if (x >= W) return;
    const float gke = g * ke;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ly = ty + 8 * i, y = y0 + ly;
        if (y >= H) break;
        const int o = y * W + x;
        const int lr = ly + 1, lc = tx + 1;
        float ga = 0.f;
        if (smooth) {
            const float gd = ((cxs[lr][lc - 1] + cxs[lr][lc + 1]) - 2.f * cxs[lr][lc]) + ((cys[lr - 1][lc] + cys[lr + 1][lc]) - 2.f * cys[lr][lc]);
            if (normalize) {
                const float s = alpha[plane + o] + M_EPS;
                if (g_depth) g_depth[plane + o] = gd / s;
                ga = -(gd * sd[ly + 2][tx + 2]) / s;
            } else if (g_depth) {
                g_depth[plane + o] = gd;
            }
            if (g_image) {
                for (int ch = 0; ch < C; ch++) {
                    const float v = si[ch][ly + 2][tx + 2];
                    const float gx = axs[lr][lc + 1] * m_sign(si[ch][ly + 2][tx + 3] - v) - axs[lr][lc] * m_sign(v - si[ch][ly + 2][tx + 1]);
                    const float gy = ays[lr + 1][lc] * m_sign(si[ch][ly + 3][tx + 2] - v) - ays[lr][lc] * m_sign(v - si[ch][ly + 1][tx + 2]);
                    g_image[plane * C + (size_t)ch * H * W + o] = gx + gy;
                }
            }
        }
        if (g_alpha) {
            if (entropy) {
                const float a = alpha[plane + o];
                if (a >= M_LO && a <= M_HI) {
                    const float t = symmetrical ? logf(1.f - a) - logf(a) : -(logf(a) + 1.f);
                    ga += gke * t;
                }
            }
            g_alpha[plane + o] = ga;
        }
    }
}

bool map_shape_ok(int64_t B, int32_t H, int32_t W) { return B >= 1 && B <= 65535 && H >= 3 && W >= 3 && (int64_t)H * W <= 0x7fffffff; }

}  // namespace

extern "C" {

int64_t nrc_map_losses_ws_floats(int64_t B, int32_t H, int32_t W) {
    if (!map_shape_ok(B, H, W)) return NRC_ERR_INVALID;
    return 4 * B * (int64_t)((W + MT_X - 1) / MT_X) * ((H + MT_Y - 1) / MT_Y) + 4;
}

int nrc_map_losses_forward(const float* depth, const float* alpha, const float* image, int64_t B, int32_t C, int32_t H, int32_t W, int32_t normalize,
                           float lambda_smooth, float lambda_entropy, int32_t symmetrical, float* workspace, float* loss4, nrc_stream_t stream) {
    NRC_ENTER();
    if (!map_shape_ok(B, H, W) || C < 1 || C > 4 || !workspace || !loss4 || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return NRC_ERR_INVALID;
    const bool smooth = lambda_smooth != 0.f, entropy = lambda_entropy != 0.f;
    if (!smooth && !entropy) return NRC_ERR_INVALID;
    if (smooth && (!depth || !image)) return NRC_ERR_INVALID;
    if (((smooth && normalize) || entropy) && !alpha) return NRC_ERR_INVALID;
    const dim3 grid((W + MT_X - 1) / MT_X, (H + MT_Y - 1) / MT_Y, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_map_fwd, grid, dim3(MT_N), 0, s, depth, alpha, image, (int)C, (int)H, (int)W, normalize ? 1 : 0, smooth ? 1 : 0, entropy ? 1 : 0,
                       symmetrical ? 1 : 0, workspace);
    const int64_t n_blocks = (int64_t)grid.x * grid.y * grid.z;
    hipLaunchKernelGGL(k_map_reduce, dim3(1), dim3(1024), 0, s, (const float*)workspace, n_blocks, 1.0 / ((double)B * H * (W - 2)), 1.0 / ((double)B * (H - 2) * W),
                       1.0 / ((double)B * H * W), lambda_smooth, lambda_entropy, loss4);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_map_losses_backward(const float* depth, const float* alpha, const float* image, int64_t B, int32_t C, int32_t H, int32_t W, int32_t normalize,
                            float lambda_smooth, float lambda_entropy, int32_t symmetrical, const float* upstream_dev, float* dL_ddepth, float* dL_dalpha,
                            float* dL_dimage, nrc_stream_t stream) {
    NRC_ENTER();
    if (!map_shape_ok(B, H, W) || C < 1 || C > 4) return NRC_ERR_INVALID;
    const bool smooth = lambda_smooth != 0.f, entropy = lambda_entropy != 0.f;
    if (!smooth && !entropy) return NRC_ERR_INVALID;
    if (!dL_ddepth && !dL_dalpha && !dL_dimage) return NRC_ERR_INVALID;
    if (smooth && (!depth || !image)) return NRC_ERR_INVALID;
    if (((smooth && normalize) || entropy) && !alpha) return NRC_ERR_INVALID;
    if (!smooth && !dL_dalpha) return NRC_ERR_INVALID;   // the entropy term has a gradient for alpha only
    const dim3 grid((W + MT_X - 1) / MT_X, (H + MT_Y - 1) / MT_Y, (unsigned)B);
    const float kx = smooth ? (float)((double)lambda_smooth / ((double)B * H * (W - 2))) : 0.f;
    const float ky = smooth ? (float)((double)lambda_smooth / ((double)B * (H - 2) * W)) : 0.f;
    const float ke = entropy ? (float)((double)lambda_entropy / ((double)B * H * W)) : 0.f;
    hipLaunchKernelGGL(k_map_bwd, grid, dim3(MT_N), 0, (hipStream_t)stream, depth, alpha, image, (int)C, (int)H, (int)W, normalize ? 1 : 0, smooth ? 1 : 0, entropy ? 1 : 0,
                       symmetrical ? 1 : 0, kx, ky, ke, upstream_dev, smooth ? dL_ddepth : (float*)nullptr, dL_dalpha, smooth ? dL_dimage : (float*)nullptr);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
