// gs_contrib.hip -- per-Gaussian contribution statistics of a rendered 3DGS view (include/nerficg_hip.h group 22): what compaction and scoring methods ask of a
// view -- the sum of blending weights, the largest blending weight and the number of pixels that blended a Gaussian.
//
// The pass runs on the state a colour forward left behind (tile lists, tile order, splat records, n_contrib): no preprocess, no sort, no binning.  For a pixel p the
// blended set and the weights are the colour pass's own, as gs_features.hip states them: the entries k <= n_contrib[p] of the tile's list with !(power > 0) and
// alpha >= 1/255, alpha = min(0.99, o exp_blend(blend_power(...))), T <- fmaf(-T, alpha, T), w = alpha T.  The alpha statements are the colour blend's own (gs_blend.h: the
// one definition gs_raster.hip includes too; replay_pack) under the one flag list of the three translation units (build.py), so w is the colour's weight bit for bit.  With m the caller's per-pixel map (1 without one) a pixel
// PARTICIPATES iff m(p) != 0, and for every Gaussian i
//     weight_sum[i] += sum_{p participates, i blended at p} m(p) w_i(p)        (f32)
//     weight_max[i]  = max(weight_max[i], max_{p participates, i blended at p} w_i(p))     (the colour's w, no rounding added)
//     hits[i]       += #{p participates : i blended at p}                      (int32, exact)
//
//   k_gs_contributions   one workgroup per tile of the band in tile_order, walking forward as the feature pass's forward kernel (gs_features.hip) does: staged batches of 256 entries, the sixteen
//                        per-4x4-block work lists, a pixel stops at its own n_contrib (0 for a pixel that does not participate), a __syncthreads_count early-out
//                        per batch.  No feature staging.  Per list entry alpha once; the 16 lanes of a DPP row (= one block = one list) reduce m w with the four
//                        dpp_add steps, w with four DPP max steps, and count themselves in the row's 16 bits of the wave's ballot.  Lane 0 of the row meets the
//                        tile's other blocks in three LDS words per batch entry: a float atomic add, an unsigned atomic max on w's bit pattern (w >= 0: the
//                        order of the patterns is the order of the values) and an integer atomic add.  One flush per batch: thread t owns entry t and adds what
//                        is not zero to the caller's buffers with at most three global atomics.
// A masked lane contributes an exact 0, 0 and 0.  weight_max is compared as a bit pattern in global memory as well: the caller's buffer holds values >= 0
// (zeros after a clear, an earlier call's maxima otherwise).
#include <hip/hip_runtime.h>

#include "common.h"
#include "gs_blend.h"

namespace {

// max(v, v of the partner lane): gs_blend.h's dpp_add with the maximum in place of the sum (same CTRL values)
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)));
}

__global__ void __launch_bounds__(256) k_gs_contributions(int W, int H, int gx, const uint32_t* __restrict__ ranges, const int32_t* __restrict__ point_list,
                                                          const float4* __restrict__ splat, const uint32_t* __restrict__ tile_order,
                                                          const uint32_t* __restrict__ n_contrib, const float* __restrict__ pixel_weights,
                                                          float* __restrict__ weight_sum, float* __restrict__ weight_max, int32_t* __restrict__ hits) {
    __shared__ StageLdsT<uint16_t> st;
    __shared__ float s_sum[BATCH];        // per batch entry, over the tile's 16 blocks: sum m w
    __shared__ uint32_t s_max[BATCH];     //                                              max w, as its bit pattern
    __shared__ int s_hits[BATCH];         //                                              blending pixels
    const int tile = (int)tile_order[blockIdx.x];
    const TilePixel tp(tile, gx, W, H);
    const int row_shift = (int)(threadIdx.x & 48u);   // this row's 16 bits of the wave's ballot
    const bool row_lead = (threadIdx.x & 15u) == 0u;
    const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
    const size_t pix = (size_t)tp.py * W + tp.px;
    const float m = tp.inside ? (pixel_weights ? pixel_weights[pix] : 1.0f) : 0.f;
    const uint32_t last = (tp.inside && m != 0.f) ? n_contrib[pix] : 0u;   // a pixel that does not participate blends nothing here
    float T = 1.0f;
    const uint2* list4 = reinterpret_cast<const uint2*>(st.list[tp.block]);
    stage_clear_records(st);
    stage_clear_lists(st);
    s_sum[threadIdx.x] = 0.f; s_max[threadIdx.x] = 0u; s_hits[threadIdx.x] = 0;
    for (uint32_t base = r0; base < r1; base += BATCH) {
        if (__syncthreads_count(base - r0 < last) == 0) break;   // no participating pixel of the tile blended anything this far back
        const uint32_t k = base + threadIdx.x;
        unsigned flags = 0u;
        int id = 0;
        if (k < r1) {
            id = point_list[k];
            flags = stage_entry<false>(st, splat, id, tp.tx0, tp.ty0);
        }
        int n_wave;
        const int n_mine = block_lists(st, flags, &n_wave);
        const uint32_t pos0 = base - r0 + 1u;  // contributor number of batch entry 0
        for (int jj = 0; jj < n_wave; jj += 4) {
            const uint2 pack = list4[jj >> 2];
            int off[4];   // 16 j
            unpack_offsets(pack, off);
            float alpha[4];
            bool ok[4];
            replay_pack(st, off, jj, n_mine, pos0, last, tp.fx, tp.fy, alpha, ok);
            if (__ballot(ok[0] | ok[1] | ok[2] | ok[3]) == 0ull) continue;   // wave-uniform
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float w = ok[u] ? alpha[u] * T : 0.f;     // an exact 0 for a masked lane
                T = ok[u] ? fmaf(-T, alpha[u], T) : T;
                const int cnt = __popc((unsigned)(__ballot(ok[u]) >> row_shift) & 0xffffu);   // the row's blending pixels
                float s = ok[u] ? m * w : 0.f, mx = w;
                s = dpp_add<0x140>(s, s); mx = dpp_max<0x140>(mx);
                s = dpp_add<0x141>(s, s); mx = dpp_max<0x141>(mx);
                s = dpp_add<0x1b>(s, s); mx = dpp_max<0x1b>(mx);
                s = dpp_add<0xb1>(s, s); mx = dpp_max<0xb1>(mx);
                if (row_lead && cnt > 0) {       // cnt > 0: some lane of the row has jj + u < n_mine, so off[u] is an entry of this row's list
                    const int j = off[u] >> 4;
                    if (weight_sum) atomicAdd(&s_sum[j], s);
                    if (weight_max) atomicMax(&s_max[j], __float_as_uint(mx));
                    if (hits) atomicAdd(&s_hits[j], cnt);
                }
            }
        }
        __syncthreads();
        // flush: thread t owns batch entry t; the next batch's LDS atomics come behind the two barriers of block_lists
        if (flags) {
            const int h = s_hits[threadIdx.x];
            const uint32_t mb = s_max[threadIdx.x];
            const float s = s_sum[threadIdx.x];
            if (h != 0) { atomicAdd(hits + id, h); s_hits[threadIdx.x] = 0; }
            if (mb != 0u) { atomicMax(reinterpret_cast<uint32_t*>(weight_max) + id, mb); s_max[threadIdx.x] = 0u; }
            if (s != 0.f) { atomicAdd(weight_sum + id, s); s_sum[threadIdx.x] = 0.f; }
        }
    }
}

// the saved state (gs_blend.h), at least one statistic asked for, and 4-byte alignment of this group's own arrays
bool contributions_args_ok(int32_t P, int32_t W, int32_t H, const int32_t* point_list, const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order,
                           const uint32_t* n_contrib, const float* pixel_weights, const float* weight_sum, const float* weight_max, const int32_t* hits,
                           int32_t tile_row_begin, int32_t n_tile_rows) {
    if (!gs_saved_state_ok(P, W, H, point_list, ranges, splat_records, tile_order, n_contrib, tile_row_begin, n_tile_rows)) return false;
    if (!weight_sum && !weight_max && !hits) return false;
    if ((reinterpret_cast<uintptr_t>(pixel_weights) | reinterpret_cast<uintptr_t>(weight_sum) | reinterpret_cast<uintptr_t>(weight_max) | reinterpret_cast<uintptr_t>(hits)) & 3u)
        return false;
    return true;
}

}  // namespace

extern "C" {

int nrc_gs_contributions_band(int32_t P, int32_t W, int32_t H, const int32_t* point_list, const uint32_t* ranges, const float* splat_records,
                              const uint32_t* tile_order, const uint32_t* n_contrib, const float* pixel_weights, float* weight_sum, float* weight_max, int32_t* hits,
                              int32_t clear, int32_t tile_row_begin, int32_t n_tile_rows, nrc_stream_t stream) {
    if (!contributions_args_ok(P, W, H, point_list, ranges, splat_records, tile_order, n_contrib, pixel_weights, weight_sum, weight_max, hits, tile_row_begin, n_tile_rows))
        return NRC_ERR_INVALID;
    NRC_ENTER();
    if (P == 0) return NRC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int gx = (W + TILE - 1) / TILE;
    NRC_STAGE(s, nullptr);
    if (clear) {
        if (weight_sum && nrc_zero_async(weight_sum, sizeof(float) * (size_t)P, s) != hipSuccess) { NRC_LAUNCH_CHECK(); return NRC_ERR_LAUNCH; }
        if (weight_max && nrc_zero_async(weight_max, sizeof(float) * (size_t)P, s) != hipSuccess) { NRC_LAUNCH_CHECK(); return NRC_ERR_LAUNCH; }
        if (hits && nrc_zero_async(hits, sizeof(int32_t) * (size_t)P, s) != hipSuccess) { NRC_LAUNCH_CHECK(); return NRC_ERR_LAUNCH; }
        NRC_STAGE(s, "zero");
    }
    // one workgroup per band tile: tile_order lists the tiles of the forward's band, so the pixels outside the band are never read
    hipLaunchKernelGGL(k_gs_contributions, dim3(gx * n_tile_rows), dim3(256), 0, s, W, H, gx, ranges, point_list, (const float4*)splat_records, tile_order, n_contrib,
                       pixel_weights, weight_sum, weight_max, hits);
    NRC_STAGE(s, "k_gs_contributions");
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
