// gs_mcmc.hip -- 3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", NeurIPS 2024) on the device: the three steps that
// replace clone / split / prune, on the raw training parameters as Gaussians stores them (o = sigmoid(logit), s = exp(log_scale), q = rotation / max(|rotation|,
// 1e-12), real part first, R = R(q) as gs_densify.hip builds it).  include/nerficg_hip.h group 16 states the formulas.
//   nrc_gs_mcmc_noise       every iteration: x += R diag(s^2) R^T (z * gate * noise_lr * lr), gate = sigmoid(100 ((1 - o) - 0.995)); z from the caller or from
//                           Philox4x32-10 keyed by (seed; global row, iteration) + Box-Muller.  One streaming pass: 44 B read + 12 B written per Gaussian, f32,
//                           no LDS, no atomics; four Gaussians per lane so that the 12-byte rows travel as 16-byte loads and stores.
//   nrc_gs_mcmc_relocation  every 100 iterations, on the rows that were drawn: opacity and scale of one Gaussian standing for N stacked copies, evaluated in
//                           f64 (the alternating binomial sum loses 1e-4 in f32) and rounded once; the drawn rows' Adam moments are cleared in the same launch.
//   nrc_gs_mcmc_regularise  the L1 regularisers on opacity and scale: gradients added in place, the two loss values from per-workgroup slabs added in f64 in a
//                           fixed order (bit-reproducible, no atomics).
// Compiled with -ffp-contract=off: the f32 sequence of the noise kernel is the one tests/gs_mcmc_ref.py counts rounding by rounding.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_ROWS = 4;            // Gaussians per lane of the noise kernel: 4 x 12 B = three 16-byte words
constexpr int MC_MOMENTS_MAX = 12;    // both Adam moments of the six parameter groups
constexpr int MC_NMAX = 50;           // the published cap on the number of stacked copies
constexpr int MC_REG_GRID_MAX = 2048; // workgroups (= slabs) of the regulariser

// Philox4x32-10 (Salmon et al. 2011): counter (c0..c3), key (k0, k1) -> four 32-bit words.  The same dozen lines as in ngp_march.hip (pinned on the
// Random123 vectors by tests/philox_ref.py), restated here so that this translation unit stands alone.
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += 0x9E3779B9u; key.y += 0xBB67AE85u;
    }
    return ctr;
}

// three standard normals of global row `index` in iteration `iteration`: counter = (index lo, index hi, iteration lo, iteration hi), key = seed;
// Box-Muller on 24-bit uniforms, the radius' uniform in (0, 1] so that the logarithm is finite: |z| <= sqrt(48 ln 2) = 5.77
__device__ __forceinline__ void draw_normals(uint64_t seed, uint64_t iteration, uint64_t index, float z[3]) {
    const uint4 w = philox4x32_10(make_uint4((uint32_t)index, (uint32_t)(index >> 32), (uint32_t)iteration, (uint32_t)(iteration >> 32)),
                                  make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    const float ua = (float)((w.x >> 8) + 1u) * 0x1p-24f, ub = (float)(w.y >> 8) * 0x1p-24f;
    const float uc = (float)((w.z >> 8) + 1u) * 0x1p-24f, ud = (float)(w.w >> 8) * 0x1p-24f;
    const float ra = sqrtf(-2.f * logf(ua)), rc = sqrtf(-2.f * logf(uc));
    float sa, ca, sc, cc;
    sincospif(2.f * ub, &sa, &ca);   // the argument in half turns: no range-reduction error of 2 pi u
    sincospif(2.f * ud, &sc, &cc);
    z[0] = ra * ca; z[1] = ra * sa; z[2] = rc * cc;
}

struct NoiseArgs {
    const float* rot; const float* log_scales; const float* logits; float* pos;
    const float* z_in; float* z_out;
    const float* lr_dev; const int32_t* device_step;
    int64_t P, row_offset;
    float noise_lr, lr;
    uint64_t seed, iteration;
};

// one Gaussian.  The f32 sequence below is the one the budget of tests/gs_mcmc_ref.py counts (B0 and the per-entry rotation terms).
__device__ __forceinline__ void noise_row(const float q_in[4], const float ls[3], float logit, const float z[3], float step, float x[3]) {
    const float o = 1.0f / (1.0f + expf(-logit));
    // 100 ((1 - o) - 0.995) = 100 (0.005 - o): the second form has no rounding of 1 - o, its error is proportional to o
    const float a = 100.0f * (0.005f - o);
    const float gate = 1.0f / (1.0f + expf(-a));
    const float v0 = (z[0] * gate) * step, v1 = (z[1] * gate) * step, v2 = (z[2] * gate) * step;
    const float s0 = expf(ls[0]), s1 = expf(ls[1]), s2 = expf(ls[2]);
    float qr = q_in[0], qi = q_in[1], qj = q_in[2], qk = q_in[3];
    const float norm = fmaxf(sqrtf(qr * qr + qi * qi + qj * qj + qk * qk), 1e-12f);
    qr /= norm; qi /= norm; qj /= norm; qk /= norm;
    const float ii2 = qi * qi * 2.f, jj2 = qj * qj * 2.f, kk2 = qk * qk * 2.f;
    const float ij2 = qi * qj * 2.f, ik2 = qi * qk * 2.f, jk2 = qj * qk * 2.f;
    const float ri2 = qr * qi * 2.f, rj2 = qr * qj * 2.f, rk2 = qr * qk * 2.f;
    const float r00 = 1.f - (jj2 + kk2), r01 = ij2 - rk2, r02 = ik2 + rj2;
    const float r10 = ij2 + rk2, r11 = 1.f - (ii2 + kk2), r12 = jk2 - ri2;
    const float r20 = ik2 - rj2, r21 = jk2 + ri2, r22 = 1.f - (ii2 + jj2);
    // R diag(s^2) R^T v: t = R^T v, u = s^2 t, d = R u
    const float t0 = r00 * v0 + r10 * v1 + r20 * v2;
    const float t1 = r01 * v0 + r11 * v1 + r21 * v2;
    const float t2 = r02 * v0 + r12 * v1 + r22 * v2;
    const float u0 = (s0 * s0) * t0, u1 = (s1 * s1) * t1, u2 = (s2 * s2) * t2;
    x[0] += r00 * u0 + r01 * u1 + r02 * u2;
    x[1] += r10 * u0 + r11 * u1 + r12 * u2;
    x[2] += r20 * u0 + r21 * u1 + r22 * u2;
}

__device__ __forceinline__ void noise_one(const NoiseArgs& a, int64_t i, uint64_t iteration, float step) {
    float q[4], ls[3], x[3], z[3];
#pragma unroll
    for (int c = 0; c < 4; c++) q[c] = a.rot[4 * i + c];
#pragma unroll
    for (int c = 0; c < 3; c++) { ls[c] = a.log_scales[3 * i + c]; x[c] = a.pos[3 * i + c]; }
    if (a.z_in) {
#pragma unroll
        for (int c = 0; c < 3; c++) z[c] = a.z_in[3 * i + c];
    } else {
        draw_normals(a.seed, iteration, (uint64_t)(a.row_offset + i), z);
    }
    noise_row(q, ls, a.logits[i], z, step, x);
#pragma unroll
    for (int c = 0; c < 3; c++) a.pos[3 * i + c] = x[c];
    if (a.z_out) {
#pragma unroll
        for (int c = 0; c < 3; c++) a.z_out[3 * i + c] = z[c];
    }
}

// VEC: every pointer is 16-byte aligned -- a lane takes four consecutive Gaussians as 16-byte words; otherwise (and for the ragged tail) one Gaussian
// per lane with 4-byte accesses.  Both run noise_row, so the result does not depend on which one a row met.
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mcmc_noise(NoiseArgs a) {
    const uint64_t iteration = a.device_step ? (uint64_t)(int64_t)*a.device_step : a.iteration;
    const float step = a.noise_lr * (a.lr_dev ? *a.lr_dev : a.lr);
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (!VEC) {
        if (t < a.P) noise_one(a, t, iteration, step);
        return;
    }
    const int64_t i0 = t * MC_ROWS;
    if (i0 >= a.P) return;
    if (i0 + MC_ROWS > a.P) {
        for (int64_t i = i0; i < a.P; i++) noise_one(a, i, iteration, step);
        return;
    }
    float q[MC_ROWS][4], ls[MC_ROWS * 3], x[MC_ROWS * 3], z[MC_ROWS * 3], lg[MC_ROWS];
    const float4* rot4 = reinterpret_cast<const float4*>(a.rot) + i0;
    const float4* ls4 = reinterpret_cast<const float4*>(a.log_scales) + 3 * t;
    float4* pos4 = reinterpret_cast<float4*>(a.pos) + 3 * t;
#pragma unroll
    for (int r = 0; r < MC_ROWS; r++) {
        const float4 v = rot4[r];
        q[r][0] = v.x; q[r][1] = v.y; q[r][2] = v.z; q[r][3] = v.w;
    }
#pragma unroll
    for (int w = 0; w < 3; w++) {
        const float4 l = ls4[w], p = pos4[w];
        ls[4 * w] = l.x; ls[4 * w + 1] = l.y; ls[4 * w + 2] = l.z; ls[4 * w + 3] = l.w;
        x[4 * w] = p.x; x[4 * w + 1] = p.y; x[4 * w + 2] = p.z; x[4 * w + 3] = p.w;
    }
    {
        const float4 l = reinterpret_cast<const float4*>(a.logits)[t];
        lg[0] = l.x; lg[1] = l.y; lg[2] = l.z; lg[3] = l.w;
    }
    if (a.z_in) {
        const float4* z4 = reinterpret_cast<const float4*>(a.z_in) + 3 * t;
#pragma unroll
        for (int w = 0; w < 3; w++) {
            const float4 v = z4[w];
            z[4 * w] = v.x; z[4 * w + 1] = v.y; z[4 * w + 2] = v.z; z[4 * w + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < MC_ROWS; r++) draw_normals(a.seed, iteration, (uint64_t)(a.row_offset + i0 + r), z + 3 * r);
    }
#pragma unroll
    for (int r = 0; r < MC_ROWS; r++) noise_row(q[r], ls + 3 * r, lg[r], z + 3 * r, step, x + 3 * r);
#pragma unroll
    for (int w = 0; w < 3; w++) pos4[w] = make_float4(x[4 * w], x[4 * w + 1], x[4 * w + 2], x[4 * w + 3]);
    if (a.z_out) {
        float4* z4 = reinterpret_cast<float4*>(a.z_out) + 3 * t;
#pragma unroll
        for (int w = 0; w < 3; w++) z4[w] = make_float4(z[4 * w], z[4 * w + 1], z[4 * w + 2], z[4 * w + 3]);
    }
}

struct MomentSet {
    float* p[MC_MOMENTS_MAX];
    int row[MC_MOMENTS_MAX];
};

// blockIdx.y == 0: the relocation arithmetic, one lane per Gaussian; blockIdx.y == 1 + t: the rows of moment tensor t with count > 0 are cleared,
// one lane per row (a few percent of the rows are drawn: the launch reads the counts once per tensor and writes only what it clears).
__global__ void __launch_bounds__(MC_THREADS) k_mcmc_relocation(float* __restrict__ logits, float* __restrict__ log_scales, const int32_t* __restrict__ count,
                                                                int64_t P, MomentSet ms, float* __restrict__ opacity_out, float* __restrict__ scales_out) {
    if (blockIdx.y > 0) {
        const int t = blockIdx.y - 1;
        const int row = ms.row[t];
        float* __restrict__ m = ms.p[t];
        for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * MC_THREADS) {
            if (count[i] <= 0) continue;
            float* __restrict__ r = m + i * row;
            for (int c = 0; c < row; c++) r[c] = 0.f;
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * MC_THREADS) {
        const int cnt = count[i];
        if (cnt <= 0) continue;
        const int N = cnt + 1 < MC_NMAX ? cnt + 1 : MC_NMAX;
        const double l = (double)logits[i];
        const double o = 1.0 / (1.0 + exp(-l));
        const double log_1mo = -log1p(exp(l));                 // ln(1 - o) without forming 1 - o
        const double o_new = -expm1(log_1mo / (double)N);      // 1 - (1 - o)^(1/N)
        // denom = sum_{i=1..N} sum_{k<i} C(i-1, k) (-1)^k / sqrt(k+1) o_new^(k+1) = sum_{k<N} C(N, k+1) (-1)^k / sqrt(k+1) o_new^(k+1): the inner sums
        // over i collapse by sum_{i=k+1..N} C(i-1, k) = C(N, k+1).  The binomials by C(N, k+1) = C(N, k) (N - k) / (k + 1): every product stays below
        // C(50, 25) * 26 < 2^53 and every quotient is an integer, so they are exact.
        double denom = 0.0, binom = 1.0, power = 1.0;
        for (int k = 0; k < N; k++) {
            binom = binom * (double)(N - k) / (double)(k + 1);
            power *= o_new;
            const double term = binom * power / sqrt((double)(k + 1));
            denom += (k & 1) ? -term : term;
        }
        const double ratio = o / denom;                        // s_new = ratio * s on all three axes
        const double log_ratio = log(ratio);
        double oc = o_new < 0.005 ? 0.005 : o_new;
        oc = oc > 1.0 - 0x1p-24 ? 1.0 - 0x1p-24 : oc;
        logits[i] = (float)log(oc / (1.0 - oc));
        if (opacity_out) opacity_out[i] = (float)oc;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double ls = (double)log_scales[3 * i + c];
            log_scales[3 * i + c] = (float)(ls + log_ratio);
            if (scales_out) scales_out[3 * i + c] = (float)(ratio * exp(ls));
        }
    }
}

// sum over the 256 lanes of a workgroup in a fixed order: lanes of a wave by xor-shuffles, the four waves one after the other
__device__ __forceinline__ double block_sum_f64(double v, double* smem) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) smem[wave] = v;
    __syncthreads();
    return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

// d logit_i += c_o o_i (1 - o_i), d log_scale_ij += c_s s_ij; slab[2 b] = the workgroup's sum of o, slab[2 b + 1] = its sum of s.  In f64: the kernel waits
// for its 48 B per Gaussian either way, and each gradient is then the correctly rounded sum of the incoming f32 value and the exact addend.
__global__ void __launch_bounds__(MC_THREADS) k_mcmc_reg(const float* __restrict__ logits, const float* __restrict__ log_scales, int64_t P, double c_o, double c_s,
                                                         float* __restrict__ grad_logits, float* __restrict__ grad_log_scales, double* __restrict__ slab) {
    __shared__ double smem[4];
    double sum_o = 0.0, sum_s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * MC_THREADS) {
        const double e = exp(-fabs((double)logits[i]));        // o (1 - o) = e / (1 + e)^2 for either sign of the logit
        const double o = logits[i] >= 0.f ? 1.0 / (1.0 + e) : e / (1.0 + e);
        sum_o += o;
        grad_logits[i] = (float)((double)grad_logits[i] + c_o * (e / ((1.0 + e) * (1.0 + e))));
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double s = exp((double)log_scales[3 * i + c]);
            sum_s += s;
            grad_log_scales[3 * i + c] = (float)((double)grad_log_scales[3 * i + c] + c_s * s);
        }
    }
    const double bo = block_sum_f64(sum_o, smem);
    const double bs = block_sum_f64(sum_s, smem);
    if (threadIdx.x == 0) { slab[2 * blockIdx.x] = bo; slab[2 * blockIdx.x + 1] = bs; }
}

// one workgroup: the slabs in a fixed order -> losses = {opacity_reg * mean(o), scale_reg * mean(s)}
__global__ void __launch_bounds__(MC_THREADS) k_mcmc_reg_finish(const double* __restrict__ slab, int n_slabs, double w_o, double w_s, float* __restrict__ losses) {
    __shared__ double smem[4];
    double a = 0.0, b = 0.0;
    for (int s = threadIdx.x; s < n_slabs; s += MC_THREADS) { a += slab[2 * s]; b += slab[2 * s + 1]; }
    a = block_sum_f64(a, smem);
    b = block_sum_f64(b, smem);
    if (threadIdx.x == 0) { losses[0] = (float)(w_o * a); losses[1] = (float)(w_s * b); }
}

int reg_slabs(int64_t P) {
    const int64_t n = nrc_cdiv(P, MC_THREADS);
    return (int)(n < 1 ? 1 : (n > MC_REG_GRID_MAX ? MC_REG_GRID_MAX : n));
}

}  // namespace

extern "C" {

int nrc_gs_mcmc_noise(const float* rotations, const float* log_scales, const float* opacity_logits, float* positions, int64_t P, int64_t row_offset,
                      float noise_lr, float lr, const float* lr_dev, uint64_t seed, uint64_t iteration, const int32_t* device_step, const float* z_in,
                      float* z_out, nrc_stream_t stream) {
    NRC_ENTER();
    if (P < 0 || row_offset < 0) return NRC_ERR_INVALID;
    if (P == 0) return NRC_OK;
    if (!rotations || !log_scales || !opacity_logits || !positions) return NRC_ERR_INVALID;
    NoiseArgs a{rotations, log_scales, opacity_logits, positions, z_in, z_out, lr_dev, device_step, P, row_offset, noise_lr, lr, seed, iteration};
    const uintptr_t bits = reinterpret_cast<uintptr_t>(rotations) | reinterpret_cast<uintptr_t>(log_scales) | reinterpret_cast<uintptr_t>(opacity_logits) |
                           reinterpret_cast<uintptr_t>(positions) | reinterpret_cast<uintptr_t>(z_in) | reinterpret_cast<uintptr_t>(z_out);
    if ((bits & 15u) == 0)
        hipLaunchKernelGGL(k_mcmc_noise<true>, dim3((unsigned)nrc_cdiv(nrc_cdiv(P, MC_ROWS), MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_mcmc_noise<false>, dim3((unsigned)nrc_cdiv(P, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, a);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_gs_mcmc_relocation(float* opacity_logits, float* log_scales, const int32_t* count, int64_t P, float* const* moments, const int32_t* moment_row_floats,
                           int32_t n_moments, float* opacity_out, float* scales_out, nrc_stream_t stream) {
    NRC_ENTER();
    if (P < 0 || n_moments < 0 || n_moments > MC_MOMENTS_MAX) return NRC_ERR_INVALID;
    if (P == 0) return NRC_OK;
    if (!opacity_logits || !log_scales || !count) return NRC_ERR_INVALID;
    if (n_moments > 0 && (!moments || !moment_row_floats)) return NRC_ERR_INVALID;
    MomentSet ms{};
    for (int t = 0; t < n_moments; t++) {
        if (!moments[t] || moment_row_floats[t] < 1) return NRC_ERR_INVALID;
        ms.p[t] = moments[t]; ms.row[t] = moment_row_floats[t];
    }
    int64_t bx = nrc_cdiv(P, MC_THREADS);
    if (bx > 65535 * 16) bx = 65535 * 16;
    hipLaunchKernelGGL(k_mcmc_relocation, dim3((unsigned)bx, (unsigned)(1 + n_moments)), dim3(MC_THREADS), 0, (hipStream_t)stream, opacity_logits, log_scales,
                       count, P, ms, opacity_out, scales_out);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int64_t nrc_gs_mcmc_regularise_ws_bytes(int64_t P) { return P < 0 ? -1 : (int64_t)reg_slabs(P) * 2 * (int64_t)sizeof(double); }

int nrc_gs_mcmc_regularise(const float* opacity_logits, const float* log_scales, int64_t P, double opacity_reg, double scale_reg, float* grad_opacity_logits,
                           float* grad_log_scales, float* losses, void* workspace, nrc_stream_t stream) {
    NRC_ENTER();
    if (P < 0) return NRC_ERR_INVALID;
    if (P == 0) return NRC_OK;
    if (!opacity_logits || !log_scales || !grad_opacity_logits || !grad_log_scales || !losses || !workspace) return NRC_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return NRC_ERR_INVALID;
    const int n_slabs = reg_slabs(P);
    const double w_o = opacity_reg / (double)P, w_s = scale_reg / (3.0 * (double)P);
    hipLaunchKernelGGL(k_mcmc_reg, dim3(n_slabs), dim3(MC_THREADS), 0, (hipStream_t)stream, opacity_logits, log_scales, P, w_o, w_s, grad_opacity_logits,
                       grad_log_scales, (double*)workspace);
    hipLaunchKernelGGL(k_mcmc_reg_finish, dim3(1), dim3(MC_THREADS), 0, (hipStream_t)stream, (const double*)workspace, n_slabs, w_o, w_s, losses);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
