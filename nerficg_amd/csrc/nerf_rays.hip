// nerf_rays.hip -- what surrounds the vanilla NeRF block in one training / rendering iteration (header group 19): stratified coarse sampling, emission-
// absorption compositing with its backward, and the fine pass's inverse-CDF resampling with the sorted union of both depth sets.  Dense: N rays x S samples,
// S the same for every ray, f32 throughout.  Reference: src/Methods/NeRF/utils.py:57-75 (generate_samples), :78-109 (generate_samples_from_pdf), :112-136
// (integrate_samples) and src/Methods/NeRF/Renderer.py:54, :70, :75 (positions = o + d t, sort(cat(t_coarse, t_fine))).
//
// WORK SPLIT.  One wave per ray, NRC_NERF_RAYS_PER_GROUP = 4 rays per workgroup (a thread per ray would leave the 1024-ray training batch on four waves of
// the whole chip).  Element-wise phases walk a ray's samples lane-strided (i = lane, lane + 64, ..: coalesced); scans give lane l the C = ceil(S / 64)
// CONSECUTIVE samples [l C, (l + 1) C), run sequentially inside the lane and combine the 64 lane totals across the wave.  Per-ray arrays are staged in LDS
// (dynamic, sized by S, at most 65 504 bytes per workgroup).  Waves behind the last ray repeat ray N - 1 without storing, so every barrier is uniform.
// No atomics, no host synchronisation, every reduction in a fixed order (two calls give the same bits; a ray's result does not depend on its neighbours).
//
// ARITHMETIC CONTRACT (built with -ffp-contract=off: every operation below rounds once, to f32; restated by tests/nerf_rays_ref.py)
//   sample_coarse   cut_k = (t_row[k+1] + t_row[k]) 0.5;  lower_i = i == 0 ? t_row[0] : cut_{i-1};  upper_i = i == S-1 ? t_row[S-1] : cut_i;
//                   t = lower + (upper - lower) u   (without u: t = t_row);   position_c = o_c + d_c t.
//   integrate       norm = sqrtf((dx dx + dy dy) + dz dz);  len_i = (t[i+1] - t[i], the last one final_delta) norm;  a_i = 1 - expf(-(sigma_i len_i)) (accurate
//                   expf);  m_i = 1 - a_i, the reference's own factor (utils.py:126: cumprod of 1 - alphas, not of the exponentials);  T_0 = 1,
//                   T_{i+1} = T_i m_i.  Order: lane chunk product p_l = ((1 m_b) m_{b+1}) .., exclusive Hillis-Steele product scan of the p_l over the lanes,
//                   then T_i = ((scan_l m_b) m_{b+1}) .. inside the chunk; T_end = T_{S-1} m_{S-1}.
//                   w_i = a_i T_i;  rgb_c = sum_i w_i c_ic (+ T_end background_c);  alpha = 1 - T_end;
//                   depth = T_end < 1 ? (sum_i w_i t_i) / alpha : 0.  Sums: lane-strided partial sums in ascending i, then a 6-step xor butterfly.
//   backward        gw_i = ((g_r c_ir + g_g c_ig) + g_b c_ib) + d_weights_i;  B = ((g_r bg_r + g_g bg_g) + g_b bg_b) - d_alpha;
//                   d_sigma_i = len_i ((gw_i (T_i m_i) - sum_{j>i} gw_j w_j) - T_end B);  d_rgb_samples_ic = w_i g_c.  T is recomputed as in the forward.  The
//                   suffix sum: lane chunk totals in ascending i, exclusive reverse Hillis-Steele scan over the lanes, then descending inside the chunk.
//                   Nothing divides by 1 - a: finite on saturated rays and with final_delta = 1e10.
//   backward_dirs   the same kernel with one more output, the gradient through |d| in len_i (group 20).  q_i = (gw_i (T_i m_i) - sum_{j>i} gw_j w_j) - T_end B is the
//                   factor whose product with len_i is d_sigma_i;  p_i = q_i (sigma_i Delta_i), Delta_i = t[i+1] - t[i], the last one final_delta;  P = sum_i p_i:
//                   lane-strided partial sums in ascending i, then the 6-step xor butterfly;  d_directions_c = (d_c / norm) P, 0 where norm = 0.  d_sigma and
//                   d_rgb_samples: the operations above, unchanged.  Where m_last = 0 (sigma_last final_delta large) q_last is 0 exactly; where sigma_last = 0 the
//                   product sigma Delta is: finite with final_delta = 1e10.  t receives no gradient, depth stays non-differentiable.
//   positions_bw    the backward of position = o + d t (group 20): d_o_c = sum_s g_sc, d_d_c = sum_s t_s g_sc (one rounded product each), both as lane-strided
//                   partial sums in ascending s starting at 0, then the 6-step xor butterfly.
//   sample_fine     knot_k = (b[k+1] + b[k]) 0.5, k < Sc-1;  mass_j = w[j+1] + 1e-5f, j < Sc-2;  total = the lanes' chunk sums (ascending j, Cm = ceil((Sc-2)/64)
//                   masses per lane) through a 6-step xor butterfly;  pdf_j = mass_j / total;  cdf[0] = 0, cdf[1+j] = P_l + r_j with r_j the running sum of
//                   lane l's chunk (ascending) and P_0 = 0, P_{l+1} = P_l + (lane l's chunk total), accumulated lane after lane: the chunk's last value IS
//                   P_{l+1}, so cdf never decreases and the search below is well defined.  right = upper_bound(cdf, u);  left = max(right-1, 0);
//                   right = min(right, Sc-2);  width = cdf[right] - cdf[left], 1 where < 1e-5f;  t_f = k0 + ((u - c0) / width) (k1 - k0).
//                   t = the ascending sort (bitonic network in LDS, padded with +inf) of the multiset t_coarse u t_fine;  position_c = o_c + d_c t.
//                   FINITE inputs are required (a NaN depth has no place in the order).
#include <math.h>

#include "common.h"

#define NRC_NERF_RAYS_PER_GROUP 4
#define NRC_NERF_RAYS_MAX_S 1024
#define NRC_NERF_RAYS_MAX_UNION 2048

namespace {

constexpr int RPG = NRC_NERF_RAYS_PER_GROUP;

__device__ __forceinline__ float wave_excl_prod(float v, int lane) {
    v = nrc_group_incl_prod<64>(v, lane);
    const float o = __shfl_up(v, 1, 64);
    return lane == 0 ? 1.f : o;
}

// sum of the values of all HIGHER lanes
__device__ __forceinline__ float wave_excl_suffix_sum(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_down(v, d, 64);
        if (lane + d < 64) v += o;
    }
    const float o = __shfl_down(v, 1, 64);
    return lane == 63 ? 0.f : o;
}

__device__ __forceinline__ float ray_norm(const float* __restrict__ d) { return sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

__device__ __forceinline__ float segment_len(const float* __restrict__ t, int i, int S, float final_delta, float norm) {
    const float delta = i + 1 < S ? t[i + 1] - t[i] : final_delta;
    return delta * norm;
}

// a[i] = 1 - expf(-(sigma_i len_i)) and T[i] = transmittance in front of sample i, for the wave's ray; returns T_end.  Called by every thread of the workgroup.
__device__ __forceinline__ float ray_transmittance(const float* __restrict__ t, const float* __restrict__ sigma, float norm, float final_delta, int S, int lane,
                                                   float* a, float* T) {
    for (int i = lane; i < S; i += 64) a[i] = 1.f - expf(-(sigma[i] * segment_len(t, i, S, final_delta, norm)));
    __syncthreads();
    const int C = (S + 63) >> 6, b = lane * C, end = min(b + C, S);
    float p = 1.f;
    for (int i = b; i < end; i++) p *= 1.f - a[i];
    float run = wave_excl_prod(p, lane);
    for (int i = b; i < end; i++) {
        T[i] = run;
        run *= 1.f - a[i];
    }
    __syncthreads();
    return T[S - 1] * (1.f - a[S - 1]);
}

__global__ void __launch_bounds__(64 * RPG) k_nerf_sample_coarse(const float* __restrict__ origins, const float* __restrict__ directions,
                                                                 const float* __restrict__ t_row, const float* __restrict__ u, int64_t N, int S,
                                                                 float* __restrict__ t_out, float* __restrict__ positions) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * RPG + (threadIdx.x >> 6);
    if (ray >= N) return;
    const float ox = origins[3 * ray], oy = origins[3 * ray + 1], oz = origins[3 * ray + 2];
    const float dx = directions[3 * ray], dy = directions[3 * ray + 1], dz = directions[3 * ray + 2];
    for (int i = lane; i < S; i += 64) {
        float t = t_row[i];
        if (u) {
            const float lower = i == 0 ? t : (t + t_row[i - 1]) * 0.5f;
            const float upper = i == S - 1 ? t : (t_row[i + 1] + t) * 0.5f;
            t = lower + (upper - lower) * u[ray * S + i];
        }
        const int64_t at = ray * S + i;
        t_out[at] = t;
        positions[3 * at] = ox + dx * t;
        positions[3 * at + 1] = oy + dy * t;
        positions[3 * at + 2] = oz + dz * t;
    }
}

__global__ void __launch_bounds__(64 * RPG) k_nerf_integrate_fw(const float* __restrict__ t, const float* __restrict__ directions, const float* __restrict__ sigma,
                                                                const float* __restrict__ rgb_in, const float* __restrict__ background, float final_delta,
                                                                int64_t N, int S, float* __restrict__ rgb_out, float* __restrict__ depth,
                                                                float* __restrict__ alpha, float* __restrict__ weights) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * RPG + wave;
    const bool valid = ray < N;
    const int64_t r = valid ? ray : N - 1;
    float* a_s = smem + (size_t)wave * 2 * S;
    float* T = a_s + S;
    const float* tr = t + r * S;
    const float T_end = ray_transmittance(tr, sigma + r * S, ray_norm(directions + 3 * r), final_delta, S, lane, a_s, T);
    float ar = 0.f, ag = 0.f, ab = 0.f, ad = 0.f;
    for (int i = lane; i < S; i += 64) {
        const float w = a_s[i] * T[i];
        const float* c = rgb_in + 3 * (r * S + i);
        if (valid) weights[r * S + i] = w;
        ar += w * c[0];
        ag += w * c[1];
        ab += w * c[2];
        ad += w * tr[i];
    }
    ar = nrc_group_sum<64>(ar);
    ag = nrc_group_sum<64>(ag);
    ab = nrc_group_sum<64>(ab);
    ad = nrc_group_sum<64>(ad);
    if (valid && lane == 0) {
        if (background) {
            ar = ar + T_end * background[0];
            ag = ag + T_end * background[1];
            ab = ab + T_end * background[2];
        }
        const float a = 1.f - T_end;
        rgb_out[3 * r] = ar;
        rgb_out[3 * r + 1] = ag;
        rgb_out[3 * r + 2] = ab;
        alpha[r] = a;
        depth[r] = T_end < 1.f ? ad / a : 0.f;
    }
}

template <bool DIRS>
__global__ void __launch_bounds__(64 * RPG) k_nerf_integrate_bw(const float* __restrict__ d_rgb, const float* __restrict__ d_alpha, const float* __restrict__ d_weights,
                                                                const float* __restrict__ t, const float* __restrict__ directions, const float* __restrict__ sigma,
                                                                const float* __restrict__ rgb_in, const float* __restrict__ background, float final_delta,
                                                                int64_t N, int S, float* __restrict__ d_sigma, float* __restrict__ d_rgb_samples,
                                                                float* __restrict__ d_directions) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * RPG + wave;
    const bool valid = ray < N;
    const int64_t r = valid ? ray : N - 1;
    float* a_s = smem + (size_t)wave * 3 * S;
    float* T = a_s + S;
    float* g = T + S;
    const float* tr = t + r * S;
    const float norm = ray_norm(directions + 3 * r);
    const float T_end = ray_transmittance(tr, sigma + r * S, norm, final_delta, S, lane, a_s, T);
    const float g0 = d_rgb ? d_rgb[3 * r] : 0.f, g1 = d_rgb ? d_rgb[3 * r + 1] : 0.f, g2 = d_rgb ? d_rgb[3 * r + 2] : 0.f;
    const float da = d_alpha ? d_alpha[r] : 0.f;
    const float B = (background ? (g0 * background[0] + g1 * background[1]) + g2 * background[2] : 0.f) - da;
    for (int i = lane; i < S; i += 64) {
        const float w = a_s[i] * T[i];
        const float* c = rgb_in + 3 * (r * S + i);
        const float gw = ((g0 * c[0] + g1 * c[1]) + g2 * c[2]) + (d_weights ? d_weights[r * S + i] : 0.f);
        g[i] = gw * w;
        if (valid) {
            float* o = d_rgb_samples + 3 * (r * S + i);
            o[0] = w * g0;
            o[1] = w * g1;
            o[2] = w * g2;
        }
    }
    __syncthreads();
    const int C = (S + 63) >> 6, b = lane * C, end = min(b + C, S);
    float tot = 0.f;
    for (int i = b; i < end; i++) tot += g[i];
    float suf = wave_excl_suffix_sum(tot, lane);
    for (int i = end - 1; i >= b; i--) {   // g[i] becomes the sum over j > i
        const float gi = g[i];
        g[i] = suf;
        suf += gi;
    }
    __syncthreads();
    const float TB = T_end * B;
    if (valid) {
        float P = 0.f;
        for (int i = lane; i < S; i += 64) {
            const float* c = rgb_in + 3 * (r * S + i);
            const float gw = ((g0 * c[0] + g1 * c[1]) + g2 * c[2]) + (d_weights ? d_weights[r * S + i] : 0.f);
            const float len = segment_len(tr, i, S, final_delta, norm);
            const float q = (gw * (T[i] * (1.f - a_s[i])) - g[i]) - TB;
            d_sigma[r * S + i] = len * q;
            if constexpr (DIRS) P += q * (sigma[r * S + i] * (i + 1 < S ? tr[i + 1] - tr[i] : final_delta));
        }
        if constexpr (DIRS) {
            P = nrc_group_sum<64>(P);
            if (lane < 3) d_directions[3 * r + lane] = norm > 0.f ? (directions[3 * r + lane] / norm) * P : 0.f;
        }
    }
}

__global__ void __launch_bounds__(64 * RPG) k_nerf_positions_bw(const float* __restrict__ d_positions, const float* __restrict__ t, int64_t N, int S,
                                                                float* __restrict__ d_origins, float* __restrict__ d_directions) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * RPG + (threadIdx.x >> 6);
    if (ray >= N) return;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
    for (int i = lane; i < S; i += 64) {
        const float* g = d_positions + 3 * (ray * S + i);
        const float ti = t[ray * S + i];
        o0 += g[0]; o1 += g[1]; o2 += g[2];
        e0 += ti * g[0]; e1 += ti * g[1]; e2 += ti * g[2];
    }
    o0 = nrc_group_sum<64>(o0); o1 = nrc_group_sum<64>(o1); o2 = nrc_group_sum<64>(o2);
    e0 = nrc_group_sum<64>(e0); e1 = nrc_group_sum<64>(e1); e2 = nrc_group_sum<64>(e2);
    if (lane == 0) {
        d_origins[3 * ray] = o0; d_origins[3 * ray + 1] = o1; d_origins[3 * ray + 2] = o2;
        d_directions[3 * ray] = e0; d_directions[3 * ray + 1] = e1; d_directions[3 * ray + 2] = e2;
    }
}

__global__ void __launch_bounds__(64 * RPG) k_nerf_sample_fine(const float* __restrict__ t_coarse, const float* __restrict__ weights, const float* __restrict__ u,
                                                               int64_t u_stride, const float* __restrict__ origins, const float* __restrict__ directions,
                                                               int64_t N, int Sc, int Sf, int P, float* __restrict__ t_out, float* __restrict__ positions,
                                                               float* __restrict__ cdf_out, float* __restrict__ t_fine_out) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * RPG + wave;
    const bool valid = ray < N;
    const int64_t r = valid ? ray : N - 1;
    const int K = Sc - 1, M = Sc - 2, n = Sc + Sf;      // knots = cdf entries, inner masses, depths of the union
    float* knots = smem + (size_t)wave * (2 * K + P);
    float* cdf = knots + K;
    float* buf = cdf + K;                                // P >= 64 floats: the lanes' totals first, the union later
    const float* tc = t_coarse + r * Sc;
    const float* w = weights + r * Sc;
    for (int k = lane; k < K; k += 64) knots[k] = (tc[k + 1] + tc[k]) * 0.5f;
    for (int j = lane; j < M; j += 64) cdf[1 + j] = w[j + 1] + 1e-5f;
    __syncthreads();
    const int Cm = (M + 63) >> 6, b = lane * Cm, end = min(b + Cm, M);
    float part = 0.f;
    for (int j = b; j < end; j++) part += cdf[1 + j];
    const float total = nrc_group_sum<64>(part);
    float run = 0.f;
    for (int j = b; j < end; j++) {
        run += cdf[1 + j] / total;
        cdf[1 + j] = run;
    }
    buf[lane] = run;
    __syncthreads();
    float acc = 0.f, mine = 0.f;
    for (int l = 0; l < 64; l++) {      // P_{l+1} = P_l + total of lane l, in lane order (see the contract: keeps cdf monotone)
        if (l == lane) mine = acc;
        acc += buf[l];
    }
    for (int j = b; j < end; j++) cdf[1 + j] = mine + cdf[1 + j];
    if (lane == 0) cdf[0] = 0.f;
    __syncthreads();
    if (valid && cdf_out)
        for (int k = lane; k < K; k += 64) cdf_out[r * K + k] = cdf[k];
    const float* ur = u + r * u_stride;
    for (int s = lane; s < Sf; s += 64) {
        const float uu = ur[s];
        int lo = 0, hi = K;
        while (lo < hi) {               // first index whose cdf is > u
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] <= uu) lo = mid + 1; else hi = mid;
        }
        const int left = max(lo - 1, 0), right = min(lo, K - 1);
        const float c0 = cdf[left], k0 = knots[left], k1 = knots[right];
        float width = cdf[right] - c0;
        if (width < 1e-5f) width = 1.f;
        const float tf = k0 + ((uu - c0) / width) * (k1 - k0);
        buf[Sc + s] = tf;
        if (valid && t_fine_out) t_fine_out[r * Sf + s] = tf;
    }
    for (int i = lane; i < Sc; i += 64) buf[i] = tc[i];
    for (int i = n + lane; i < P; i += 64) buf[i] = INFINITY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = lane; idx < (P >> 1); idx += 64) {
                const int lo = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), hi = lo | j;
                const float a = buf[lo], c = buf[hi];
                if ((a > c) == ((lo & k) == 0)) {
                    buf[lo] = c;
                    buf[hi] = a;
                }
            }
            __syncthreads();
        }
    if (valid) {
        const float ox = origins[3 * r], oy = origins[3 * r + 1], oz = origins[3 * r + 2];
        const float dx = directions[3 * r], dy = directions[3 * r + 1], dz = directions[3 * r + 2];
        for (int i = lane; i < n; i += 64) {
            const float t = buf[i];
            const int64_t at = r * n + i;
            t_out[at] = t;
            positions[3 * at] = ox + dx * t;
            positions[3 * at + 1] = oy + dy * t;
            positions[3 * at + 2] = oz + dz * t;
        }
    }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
inline bool s_ok(int64_t S) { return S >= 1 && S <= NRC_NERF_RAYS_MAX_S; }
inline bool fine_ok(int64_t Sc, int64_t Sf) { return Sc >= 3 && Sc <= NRC_NERF_RAYS_MAX_S && Sf >= 1 && Sf <= NRC_NERF_RAYS_MAX_S && Sc + Sf <= NRC_NERF_RAYS_MAX_UNION; }

}  // namespace

extern "C" {

int nrc_nerf_rays_per_group(void) { return NRC_NERF_RAYS_PER_GROUP; }

int nrc_nerf_rays_supported(int32_t S_coarse, int32_t S_fine) { return S_fine == 0 ? (s_ok(S_coarse) ? 1 : 0) : (fine_ok(S_coarse, S_fine) ? 1 : 0); }

int nrc_nerf_sample_coarse(const float* origins, const float* directions, const float* t_row, const float* u, int64_t N, int32_t S, float* t,
                           float* positions, nrc_stream_t stream) {
    NRC_ENTER();
    if (!s_ok(S)) return NRC_ERR_UNSUPPORTED;
    if (N < 0) return NRC_ERR_INVALID;
    if (N == 0) return NRC_OK;
    if (!origins || !directions || !t_row || !t || !positions || misaligned(origins) || misaligned(directions) || misaligned(t_row) || misaligned(u) ||
        misaligned(t) || misaligned(positions)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(N, RPG);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    NRC_STAGE(s, nullptr);
    hipLaunchKernelGGL(k_nerf_sample_coarse, dim3((unsigned)blocks), dim3(64 * RPG), 0, s, origins, directions, t_row, u, N, (int)S, t, positions);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_sample_coarse");
    return NRC_OK;
}

int nrc_nerf_integrate_forward(const float* t, const float* directions, const float* sigma, const float* rgb_samples, const float* background,
                               float final_delta, int64_t N, int32_t S, float* rgb, float* depth, float* alpha, float* weights, nrc_stream_t stream) {
    NRC_ENTER();
    if (!s_ok(S)) return NRC_ERR_UNSUPPORTED;
    if (N < 0) return NRC_ERR_INVALID;
    if (N == 0) return NRC_OK;
    if (!t || !directions || !sigma || !rgb_samples || !rgb || !depth || !alpha || !weights || misaligned(t) || misaligned(directions) || misaligned(sigma) ||
        misaligned(rgb_samples) || misaligned(background) || misaligned(rgb) || misaligned(depth) || misaligned(alpha) || misaligned(weights))
        return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(N, RPG);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    NRC_STAGE(s, nullptr);
    hipLaunchKernelGGL(k_nerf_integrate_fw, dim3((unsigned)blocks), dim3(64 * RPG), (size_t)RPG * 2 * S * sizeof(float), s, t, directions, sigma, rgb_samples,
                       background, final_delta, N, (int)S, rgb, depth, alpha, weights);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_integrate_fw");
    return NRC_OK;
}

int nrc_nerf_integrate_backward(const float* d_rgb, const float* d_alpha, const float* d_weights, const float* t, const float* directions, const float* sigma,
                                const float* rgb_samples, const float* background, float final_delta, int64_t N, int32_t S, float* d_sigma,
                                float* d_rgb_samples, nrc_stream_t stream) {
    NRC_ENTER();
    if (!s_ok(S)) return NRC_ERR_UNSUPPORTED;
    if (N < 0) return NRC_ERR_INVALID;
    if (N == 0) return NRC_OK;
    if (!t || !directions || !sigma || !rgb_samples || !d_sigma || !d_rgb_samples || misaligned(d_rgb) || misaligned(d_alpha) || misaligned(d_weights) ||
        misaligned(t) || misaligned(directions) || misaligned(sigma) || misaligned(rgb_samples) || misaligned(background) || misaligned(d_sigma) ||
        misaligned(d_rgb_samples)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(N, RPG);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    NRC_STAGE(s, nullptr);
    hipLaunchKernelGGL(k_nerf_integrate_bw<false>, dim3((unsigned)blocks), dim3(64 * RPG), (size_t)RPG * 3 * S * sizeof(float), s, d_rgb, d_alpha, d_weights, t,
                       directions, sigma, rgb_samples, background, final_delta, N, (int)S, d_sigma, d_rgb_samples, (float*)nullptr);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_integrate_bw");
    return NRC_OK;
}

int nrc_nerf_sample_fine(const float* t_coarse, const float* weights, const float* u, int64_t u_stride, const float* origins, const float* directions,
                         int64_t N, int32_t S_coarse, int32_t S_fine, float* t, float* positions, float* cdf, float* t_fine, nrc_stream_t stream) {
    NRC_ENTER();
    if (!fine_ok(S_coarse, S_fine)) return NRC_ERR_UNSUPPORTED;
    if (N < 0 || (u_stride != 0 && u_stride < S_fine)) return NRC_ERR_INVALID;
    if (N == 0) return NRC_OK;
    if (!t_coarse || !weights || !u || !origins || !directions || !t || !positions || misaligned(t_coarse) || misaligned(weights) || misaligned(u) ||
        misaligned(origins) || misaligned(directions) || misaligned(t) || misaligned(positions) || misaligned(cdf) || misaligned(t_fine)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(N, RPG);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    int P = 64;                                         // the sorting network's size; its first 64 floats also carry the lanes' totals
    while (P < S_coarse + S_fine) P <<= 1;
    const size_t lds = (size_t)RPG * (2 * (S_coarse - 1) + P) * sizeof(float);   // <= 4 (2 x 1023 + 2048) x 4 = 65 504 bytes
    hipStream_t s = (hipStream_t)stream;
    NRC_STAGE(s, nullptr);
    hipLaunchKernelGGL(k_nerf_sample_fine, dim3((unsigned)blocks), dim3(64 * RPG), lds, s, t_coarse, weights, u, u_stride, origins, directions, N, (int)S_coarse,
                       (int)S_fine, P, t, positions, cdf, t_fine);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_sample_fine");
    return NRC_OK;
}

int nrc_nerf_integrate_backward_dirs(const float* d_rgb, const float* d_alpha, const float* d_weights, const float* t, const float* directions,
                                     const float* sigma, const float* rgb_samples, const float* background, float final_delta, int64_t N, int32_t S,
                                     float* d_sigma, float* d_rgb_samples, float* d_directions, nrc_stream_t stream) {
    NRC_ENTER();
    if (!s_ok(S)) return NRC_ERR_UNSUPPORTED;
    if (N < 0) return NRC_ERR_INVALID;
    if (N == 0) return NRC_OK;
    if (!t || !directions || !sigma || !rgb_samples || !d_sigma || !d_rgb_samples || !d_directions || misaligned(d_rgb) || misaligned(d_alpha) ||
        misaligned(d_weights) || misaligned(t) || misaligned(directions) || misaligned(sigma) || misaligned(rgb_samples) || misaligned(background) ||
        misaligned(d_sigma) || misaligned(d_rgb_samples) || misaligned(d_directions)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(N, RPG);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    NRC_STAGE(s, nullptr);
    hipLaunchKernelGGL(k_nerf_integrate_bw<true>, dim3((unsigned)blocks), dim3(64 * RPG), (size_t)RPG * 3 * S * sizeof(float), s, d_rgb, d_alpha, d_weights, t,
                       directions, sigma, rgb_samples, background, final_delta, N, (int)S, d_sigma, d_rgb_samples, d_directions);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_integrate_bw_dirs");
    return NRC_OK;
}

int nrc_nerf_positions_backward(const float* d_positions, const float* t, int64_t N, int32_t S, float* d_origins, float* d_directions, nrc_stream_t stream) {
    NRC_ENTER();
    if (!s_ok(S)) return NRC_ERR_UNSUPPORTED;
    if (N < 0) return NRC_ERR_INVALID;
    if (N == 0) return NRC_OK;
    if (!d_positions || !t || !d_origins || !d_directions || misaligned(d_positions) || misaligned(t) || misaligned(d_origins) || misaligned(d_directions))
        return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(N, RPG);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    NRC_STAGE(s, nullptr);
    hipLaunchKernelGGL(k_nerf_positions_bw, dim3((unsigned)blocks), dim3(64 * RPG), 0, s, d_positions, t, N, (int)S, d_origins, d_directions);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_positions_bw");
    return NRC_OK;
}

}  // extern "C"
