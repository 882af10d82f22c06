// gs_features.hip -- N-channel per-Gaussian features blended by the 3DGS rasterizer's own weights, forward and backward (include/nerficg_hip.h group 21).
//
// A feature pass runs on the state a colour forward left behind (tile lists, tile order, splat records, n_contrib, final_T): no preprocess, no sort,
// no binning.  For a pixel p the blended set and the weights are the colour pass's own: the entries k <= n_contrib[p] of the tile's list with
// !(power > 0) and alpha >= 1/255, alpha = min(0.99, o exp_blend(blend_power(...))), T <- fmaf(-T, alpha, T), w = alpha T; the map is
// F_c = fmaf(f_c, w, F_c) in list order, background 0, not normalised.  The alpha statements are the colour blend's own -- gs_blend.h holds the one definition that
// gs_raster.hip includes too, the forward kernel walks a batch through its replay_pack -- and the three translation units share one flag list (build.py), so w is
// the colour's weight bit for bit: a feature column that holds a colour gives that colour's plane (bg = 0) bitwise.
//
//   k_render_features<CH>     one workgroup per (tile of the band in tile_order, chunk of CH channels); the per-4x4-block work lists of the colour blend; a batch's
//                             256 x CH features staged in LDS (16 KB at CH = 16, read back as 16-byte vectors); alpha once per entry, CH multiply-adds.
//                             A pixel stops at its own n_contrib: no saturation test.
//   k_render_features_bw<CH>  the same tiles and chunks, back to front from final_T as the colour blend backward walks: per pixel n_c (what lies behind) and g_c in registers,
//                                 dL/df[i, c]  = sum_p w_i g_c            dL/dalpha_i(p) = T_i sum_c (f[i, c] - n_c) g_c            n_c <- alpha f_c + (1 - alpha) n_c
//                             (no background term), dL/dalpha on to opacity, mean2D and conic as for a colour.  The CH feature sums of a row of 16 lanes are
//                             reduced by a transposing DPP exchange (15 adds, the sum of column c ends in lane c), the six geometry sums by a second one
//                             (8 adds); both meet the tile's other blocks in LDS as f32 atomics and are flushed once per batch: one contiguous group of CH
//                             floats per Gaussian into dL_dfeatures, six floats into slots [3..8] of the Gaussian's 64-byte gradient record.
// C > CH: the chunk is the grid's second dimension (one launch); every chunk recomputes alpha and adds its own share of the geometry sums, which are
// linear in the channels.  Accumulation is f32 throughout: tests/gs_features_ref.py states its error.
#include <hip/hip_runtime.h>

#include "common.h"
#include "gs_blend.h"

#define FEAT_CH 16
#define FEAT_C_MAX 256

namespace {

// features of entry `id`, channels [c0, c0 + nch) -> v[CH] (zero behind nch).  vec4: C % 4 == 0 and a 16-byte aligned base, so every chunk row is too
template <int CH>
__device__ __forceinline__ void load_feature_chunk(const float* __restrict__ features, int id, int C, int c0, int nch, int vec4, float (&v)[CH]) {
    const float* fr = features + (size_t)id * (size_t)C + c0;
    if (vec4) {
#pragma unroll
        for (int g = 0; g < CH / 4; g++) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * g < nch) q = reinterpret_cast<const float4*>(fr)[g];
            v[4 * g] = q.x; v[4 * g + 1] = q.y; v[4 * g + 2] = q.z; v[4 * g + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CH; k++) v[k] = k < nch ? fr[k] : 0.f;
    }
}

template <int CH>
__global__ void __launch_bounds__(256) k_render_features(int W, int H, int gx, int C, int vec4, const float* __restrict__ features, const uint32_t* __restrict__ ranges,
                                                         const int32_t* __restrict__ point_list, const float4* __restrict__ splat,
                                                         const uint32_t* __restrict__ tile_order, const uint32_t* __restrict__ n_contrib,
                                                         float* __restrict__ out) {
    static_assert(CH % 4 == 0, "chunks are staged as 16-byte vectors");
    __shared__ StageLdsT<uint16_t> st;
    __shared__ float4 s_f[BATCH][CH / 4];
    const int tile = (int)tile_order[blockIdx.x];
    const int c0 = (int)blockIdx.y * CH;
    const int nch = min(CH, C - c0);
    const TilePixel tp(tile, gx, W, H);
    const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
    const size_t pix = (size_t)tp.py * W + tp.px, hw = (size_t)H * W;
    const uint32_t last = tp.inside ? n_contrib[pix] : 0u;   // contributor number of the last entry the colour pass blended here
    float T = 1.0f;
    float F[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) F[k] = 0.f;
    const uint2* list4 = reinterpret_cast<const uint2*>(st.list[tp.block]);
    stage_clear_records(st);
#pragma unroll
    for (int g = 0; g < CH / 4; g++) s_f[threadIdx.x][g] = make_float4(0.f, 0.f, 0.f, 0.f);   // the staged features of a stale offset: finite too
    stage_clear_lists(st);
    for (uint32_t base = r0; base < r1; base += BATCH) {
        if (__syncthreads_count(base - r0 < last) == 0) break;   // no pixel of the tile blended anything this far back
        const uint32_t k = base + threadIdx.x;
        unsigned flags = 0u;
        if (k < r1) {
            const int id = point_list[k];
            flags = stage_entry<false>(st, splat, id, tp.tx0, tp.ty0);
            if (flags) {
                float v[CH];
                load_feature_chunk<CH>(features, id, C, c0, nch, vec4, v);
#pragma unroll
                for (int g = 0; g < CH / 4; g++) s_f[threadIdx.x][g] = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
            }
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
                const float w = ok[u] ? alpha[u] * T : 0.f;     // an exact 0 for a masked lane; the features it multiplies are finite
                T = ok[u] ? fmaf(-T, alpha[u], T) : T;
                const float4* fp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_f) + (CH / 4) * off[u]);
#pragma unroll
                for (int g = 0; g < CH / 4; g++) {
                    const float4 q = fp[g];
                    F[4 * g] = fmaf(q.x, w, F[4 * g]); F[4 * g + 1] = fmaf(q.y, w, F[4 * g + 1]);
                    F[4 * g + 2] = fmaf(q.z, w, F[4 * g + 2]); F[4 * g + 3] = fmaf(q.w, w, F[4 * g + 3]);
                }
            }
        }
        __syncthreads();
    }
    if (tp.inside) {
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (k < nch) out[(size_t)(c0 + k) * hw + pix] = F[k];
    }
}

// One exchange step of the transposing row reduction: of v[0 .. 2 n) a lane keeps the upper half when `upper` and the lower half otherwise, and adds what its
// partner (which keeps the other half) held of it.  The partner's `upper` is the opposite.
template <int CTRL, int N>
__device__ __forceinline__ void transpose_step(float* v, bool upper) {
#pragma unroll
    for (int i = 0; i < N; i++) {
        const float keep = upper ? v[N + i] : v[i], send = upper ? v[i] : v[N + i];
        v[i] = dpp_add<CTRL>(keep, send);
    }
}

template <int CH>
__global__ void __launch_bounds__(256) k_render_features_bw(int W, int H, int gx, int C, int vec4, const float* __restrict__ features, const uint32_t* __restrict__ ranges,
                                                            const int32_t* __restrict__ point_list, const float4* __restrict__ splat,
                                                            const uint32_t* __restrict__ tile_order, const uint32_t* __restrict__ n_contrib,
                                                            const float* __restrict__ final_T, const float* __restrict__ dL_dmap, float* __restrict__ dL_dfeatures,
                                                            float* __restrict__ grad_rec) {
    static_assert(CH == 16, "the transposing reduction leaves column c in lane c of a 16-lane row");
    __shared__ StageLdsT<uint8_t> st;
    __shared__ float4 s_f[BATCH][CH / 4];
    __shared__ float s_accF[BATCH][CH];   // per-Gaussian feature sums of the tile's 16 blocks, flushed once per batch
    __shared__ float s_accG[BATCH][8];    // opacity, mean x, mean y, conic xx, xy, yy, -, -
    __shared__ int s_id[BATCH];           // Gaussian of batch entry t (-1: nothing staged)
    __shared__ int s_blast[N_BLOCKS];
    const int tile = (int)tile_order[blockIdx.x];
    const int c0 = (int)blockIdx.y * CH;
    const int nch = min(CH, C - c0);
    const int tile_x = tile % gx, tile_y = tile / gx;
    const int lane = threadIdx.x & 63;
    const int block = threadIdx.x >> 4;
    const float tx0 = (float)(tile_x * TILE), ty0 = (float)(tile_y * TILE);
    const int px = tile_x * TILE + tile_px(threadIdx.x), py = tile_y * TILE + tile_py(threadIdx.x);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;
    const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
    const int n_tile = (int)(r1 - r0);
    const size_t pix = (size_t)py * W + px, hw = (size_t)H * W;
    float T = inside ? final_T[pix] : 0.f;
    const int last = inside ? (int)n_contrib[pix] : 0;
    float n[CH], g[CH];   // what lies behind the current Gaussian; the pixel's gradients
    bool any = false;
#pragma unroll
    for (int k = 0; k < CH; k++) {
        n[k] = 0.f;
        g[k] = (inside && k < nch) ? dL_dmap[(size_t)(c0 + k) * hw + pix] : 0.f;
        any = any | (g[k] != 0.f);
    }
    int block_last = last;
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) block_last = max(block_last, __shfl_xor(block_last, d, 16));
    if ((threadIdx.x & 15) == 0) s_blast[block] = block_last;
    st.a[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f); st.b[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < CH / 4; q++) s_f[threadIdx.x][q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!__syncthreads_or(any)) return;   // no gradient of this chunk reaches this tile (uniform over the workgroup)
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;
    const int l16 = lane & 15;
    const bool b3 = l16 & 8, b2 = l16 & 4, b1 = l16 & 2, b0 = l16 & 1;
    const int g_col = (b3 ? 4 : 0) + (b2 ? 2 : 0) + (b1 ? 1 : 0);   // the geometry column lanes (2 c, 2 c + 1) end up with
    const int blast_v = lane < N_BLOCKS ? s_blast[lane] : 0;  // lanes 0..15 of every wave: the 16 block maxima
    int n_eff = blast_v;
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) n_eff = max(n_eff, __shfl_xor(n_eff, d, 16));
    n_eff = min(n_tile, __builtin_amdgcn_readfirstlane(n_eff));
    const uint32_t* list4 = reinterpret_cast<const uint32_t*>(st.list[block]);
    // batches are taken from the END of the blended prefix, as in the colour blend backward: batch entry t sits at list position n_eff - 1 - done_cnt - t
    for (int done_cnt = 0; done_cnt < n_eff; done_cnt += BATCH) {
        __syncthreads();
        const int nb_raw = min(BATCH, n_eff - done_cnt);
#pragma unroll
        for (int q = 0; q < CH; q++) s_accF[threadIdx.x][q] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; q++) s_accG[threadIdx.x][q] = 0.f;
        int id_l = 0;
        unsigned flags = 0;
        const int pos_top = n_eff - 1 - done_cnt;  // list position of batch entry 0
        if ((int)threadIdx.x < nb_raw) {
            id_l = point_list[r0 + pos_top - threadIdx.x];
            const float4* rec = splat + 4 * (size_t)id_l;
            const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
            flags = block_flags(q0, q1, q2, tx0, ty0);
            const int pos_l = pos_top - (int)threadIdx.x;
#pragma unroll
            for (int b = 0; b < N_BLOCKS; b++)  // no pixel of block b blended anything at or behind its maximum
                if (pos_l >= __builtin_amdgcn_readlane(blast_v, b)) flags &= ~(1u << b);
            if (flags) {
                st.a[threadIdx.x] = make_float4(q0.x, q0.y, 0.f, 0.f);
                st.b[threadIdx.x] = make_float4(q0.z, q1.x, q0.w, q1.y);
                float v[CH];
                load_feature_chunk<CH>(features, id_l, C, c0, nch, vec4, v);
#pragma unroll
                for (int q = 0; q < CH / 4; q++) s_f[threadIdx.x][q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            }
        }
        s_id[threadIdx.x] = flags ? id_l : -1;
        int n_wave;
        const int n_mine = block_lists(st, flags, &n_wave);
        // entry j of the batch sits at list position pos_top - j; this pixel blended the positions < last: j > pos_top - last
        const int j_behind = pos_top - last;
        for (int jj = 0; jj < n_wave; jj++) {
            const uint32_t pack = list4[jj >> 2];  // four entries of this row's list per dword
            const int j = (int)__builtin_amdgcn_ubfe(pack, 8u * ((uint32_t)jj & 3u), 8u);
            const float4 co = st.b[j];             // A, C, B, o
            const float4 xy = st.a[j];
            const v2f d = (v2f){xy.x, xy.y} - (v2f){fx, fy};
            const float power = blend_power((v2f){co.x, co.y}, co.z, d);
            const float G = exp_blend(power);
            const float alpha = fminf(0.99f, co.w * G);   // exactly as the forward computed it
            const bool active = (jj < n_mine) & (j > j_behind) & !(power > 0.0f) & !(alpha < 1.0f / 255.0f);
            if (__ballot(active) == 0ull) continue;  // nobody in this wave sees its Gaussian (wave-uniform: the exchanges below run with every lane)
            // two masked factors carry `active`: a lane that does not blend this Gaussian multiplies T by 1, moves n by 0 and adds 0 to every sum
            const float alpha_m = active ? alpha : 0.f, Gm = active ? G : 0.f;
            const float r_om = __builtin_amdgcn_rcpf(1 - alpha_m);
            const float T_new = T * r_om;            // the transmittance in front of this Gaussian
            const float dchm = alpha_m * T_new;      // its weight w = alpha T
            float v[CH];
            float dL_dalpha = 0.f;
#pragma unroll
            for (int q = 0; q < CH / 4; q++) {
                const float4 f4 = s_f[j][q];
                const float fv[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int c = 4 * q + t;
                    const float e = fv[t] - n[c];                      // the feature of this Gaussian minus what lies behind it
                    dL_dalpha = c == 0 ? e * g[0] : fmaf(e, g[c], dL_dalpha);
                    n[c] = fmaf(alpha_m, e, n[c]);                     // = alpha f + (1 - alpha) n
                    v[c] = dchm * g[c];
                }
            }
            dL_dalpha = dL_dalpha * T_new;
            T = T_new;
            const float d_op = Gm * dL_dalpha;          // sum G dL/dalpha
            const float wgt = co.w * d_op;              // G dL/dG
            const float wx = wgt * d.x, wy = wgt * d.y;
            float s[8];
            s[0] = d_op;
            s[1] = fmaf(wx, co.x, wy * co.z); s[2] = fmaf(wy, co.y, wx * co.z);   // flushed with -0.5 W, -0.5 H
            s[3] = wx * d.x; s[4] = wx * d.y; s[5] = wy * d.y;                      // flushed with -1/2
            s[6] = 0.f; s[7] = 0.f;
            // transposing row reductions (row = block = one Gaussian): partners lane ^ 15, ^ 7, ^ 3, ^ 1; a lane keeps one half of its values per step
            transpose_step<0x140, 8>(v, b3);
            transpose_step<0x141, 4>(v, b2);
            transpose_step<0x1b, 2>(v, b1);
            transpose_step<0xb1, 1>(v, b0);             // v[0] = the row's sum of column l16
            transpose_step<0x140, 4>(s, b3);
            transpose_step<0x141, 2>(s, b2);
            transpose_step<0x1b, 1>(s, b1);
            const float gsum = dpp_add<0xb1>(s[0], s[0]);   // column g_col in both lanes of the pair
            if (jj < n_mine) {
                atomicAdd(&s_accF[j][l16], v[0]);
                if (!b0 && g_col < 6) atomicAdd(&s_accG[j][g_col], gsum);
            }
        }
        __syncthreads();
        // Flush: the 16 lanes of a DPP row take ONE batch entry -- a wave-instruction adds four contiguous groups of CH floats, each one Gaussian's
        // row chunk of dL_dfeatures, and four 24-byte groups inside four gradient records.
        {
            const int q = threadIdx.x & 15;
            const float gs = q == 0 ? 1.0f : q == 1 ? -ddelx_dx : q == 2 ? -ddely_dy : -0.5f;
            for (int e = threadIdx.x >> 4; e < nb_raw; e += 16) {
                const int id = s_id[e];
                if (id >= 0) {
                    if (dL_dfeatures && q < nch) {
                        const float a = s_accF[e][q];
                        if (a != 0.f) atomicAdd(dL_dfeatures + (size_t)id * (size_t)C + c0 + q, a);
                    }
                    if (q < 6) {
                        const float a = s_accG[e][q];
                        if (a != 0.f) atomicAdd(grad_rec + (size_t)id * GREC + 3 + q, a * gs);
                    }
                }
            }
        }
    }
}

// the saved state (gs_blend.h) and the feature table
bool features_args_ok(int32_t P, int32_t C, int32_t W, int32_t H, const float* features, const int32_t* point_list, const uint32_t* ranges, const float* splat_records,
                      const uint32_t* tile_order, const uint32_t* n_contrib, int32_t tile_row_begin, int32_t n_tile_rows) {
    if (!gs_saved_state_ok(P, W, H, point_list, ranges, splat_records, tile_order, n_contrib, tile_row_begin, n_tile_rows)) return false;
    if (C < 1 || C > FEAT_C_MAX || (P > 0 && !features)) return false;
    return (reinterpret_cast<uintptr_t>(features) & 3u) == 0;
}
int features_vec4(int32_t C, const float* features) { return (C % 4 == 0 && (reinterpret_cast<uintptr_t>(features) & 15u) == 0) ? 1 : 0; }

}  // namespace

extern "C" {

int nrc_gs_render_features_band(int32_t P, int32_t C, int32_t W, int32_t H, const float* features, const int32_t* point_list, const uint32_t* ranges,
                                const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib, int32_t tile_row_begin, int32_t n_tile_rows,
                                float* out_features, nrc_stream_t stream) {
    if (!features_args_ok(P, C, W, H, features, point_list, ranges, splat_records, tile_order, n_contrib, tile_row_begin, n_tile_rows) || !out_features)
        return NRC_ERR_INVALID;
    NRC_ENTER();
    hipStream_t s = (hipStream_t)stream;
    const int gx = (W + TILE - 1) / TILE;
    NRC_STAGE(s, nullptr);
    // one workgroup per (band tile, chunk): tile_order lists the tiles of the forward's band, so the pixel rows outside the band are never written.
    // P == 0: every list is empty and the band's pixels receive zeros.
    hipLaunchKernelGGL(k_render_features<FEAT_CH>, dim3(gx * n_tile_rows, (unsigned)nrc_cdiv(C, FEAT_CH)), dim3(256), 0, s, W, H, gx, C, features_vec4(C, features), features,
                       ranges, point_list, (const float4*)splat_records, tile_order, n_contrib, out_features);
    NRC_STAGE(s, "k_render_features");
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_gs_backward_features_band(int32_t P, int32_t C, int32_t W, int32_t H, const float* features, const int32_t* point_list, const uint32_t* ranges,
                                  const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib, const float* final_T,
                                  const float* dL_dfeature_map, float* dL_dfeatures, float* grad_records, int32_t records_clear, int32_t tile_row_begin,
                                  int32_t n_tile_rows, nrc_stream_t stream) {
    if (!features_args_ok(P, C, W, H, features, point_list, ranges, splat_records, tile_order, n_contrib, tile_row_begin, n_tile_rows) || !final_T || !dL_dfeature_map)
        return NRC_ERR_INVALID;
    if ((P > 0 && !grad_records) || (reinterpret_cast<uintptr_t>(grad_records) & 63u) || (reinterpret_cast<uintptr_t>(dL_dfeatures) & 3u)) return NRC_ERR_INVALID;
    NRC_ENTER();
    if (P == 0) return NRC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int gx = (W + TILE - 1) / TILE;
    NRC_STAGE(s, nullptr);
    if (!records_clear && nrc_zero_async(grad_records, sizeof(float) * GREC * (size_t)P, s) != hipSuccess) { NRC_LAUNCH_CHECK(); return NRC_ERR_LAUNCH; }
    if (dL_dfeatures && nrc_zero_async(dL_dfeatures, sizeof(float) * (size_t)P * (size_t)C, s) != hipSuccess) { NRC_LAUNCH_CHECK(); return NRC_ERR_LAUNCH; }
    NRC_STAGE(s, "zero");
    hipLaunchKernelGGL(k_render_features_bw<FEAT_CH>, dim3(gx * n_tile_rows, (unsigned)nrc_cdiv(C, FEAT_CH)), dim3(256), 0, s, W, H, gx, C, features_vec4(C, features), features,
                       ranges, point_list, (const float4*)splat_records, tile_order, n_contrib, final_T, dL_dfeature_map, dL_dfeatures, grad_records);
    NRC_STAGE(s, "k_render_features_bw");
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
