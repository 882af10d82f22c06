// gs_blend.h -- the blend kernels' shared statements, for translation units beside gs_raster.hip (gs_features.hip).
//
// These are COPIES, statement for statement, of what the colour blend / the colour blend backward use in gs_raster.hip (section 5, "render"): the pixel layout of a tile, the
// conservative per-block test, the exponent, the exponential, the staged batch and its sixteen per-block work lists, and the DPP exchange-and-add.
// gs_raster.hip keeps its own text, so none of its kernels changes with this file.  A kernel that includes this header and is built with gs_raster.hip's
// flags (-ffp-contract=off -fno-slp-vectorize, no atomic optimizer) computes alpha -- hence the blended set and every weight alpha T -- bit for bit
// as the colour pass does.  The reasons behind each statement are written down at the originals; whoever changes one side changes the other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TILE 16
#define BATCH 256
#define N_BLOCKS 16
#define GREC 16   // floats of a gradient record: [0..2] colour  [3] opacity  [4..5] mean2D  [6..8] conic xx, xy, yy  [9] dz  [10..15] unused

namespace {

// thread -> pixel of the 16x16 tile: wave = 8x8 quadrant, DPP row (16 lanes) = 4x4 block of the quadrant; block index b = 4 * wave + row
__device__ __forceinline__ int tile_px(unsigned t) { return (int)((t & 3u) + ((t >> 4) & 1u) * 4u + ((t >> 6) & 1u) * 8u); }
__device__ __forceinline__ int tile_py(unsigned t) { return (int)(((t >> 2) & 3u) + ((t >> 5) & 1u) * 4u + (t >> 7) * 8u); }

// bit b set when the alpha >= 1/255 ellipse of the record can reach a pixel centre of block b (conservative: bounding box, then chords per row band)
__device__ __forceinline__ unsigned block_flags(const float4& q0, const float4& q1, const float4& q2, float tx0, float ty0) {
    const float X = q0.x, Y = q0.y, ex = q1.z, ey = q1.w;
    if (!(ex >= 0.f)) return 0u;  // never reaches the threshold
    unsigned col = 0, row = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float x0 = tx0 + (float)(4 * c), y0 = ty0 + (float)(4 * c);
        col |= (unsigned)(X + ex >= x0 && X - ex <= x0 + 3.f) << c;
        row |= (unsigned)(Y + ey >= y0 && Y - ey <= y0 + 3.f) << c;
    }
    if (col == 0u || row == 0u) return 0u;
    unsigned cols[4] = {col, col, col, col};
    if (ex < __builtin_inff()) {
        const float ta = q2.x, da = q2.y, ba = q2.z, yoff = q2.w;   // half chord at offset d from the centre row: sqrt(tau / A - (det / A^2) d^2)
        float lo[5], hi[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const float d = fminf(fmaxf(Y - (ty0 + (float)(4 * k)), -ey), ey);
            const float w = __builtin_amdgcn_sqrtf(fmaxf(ta - da * d * d, 0.f));
            const float mid = X + ba * d;
            lo[k] = mid - w; hi[k] = mid + w;
        }
        const float yl = Y + yoff, yr = Y - yoff;
#pragma unroll
        for (int sl = 0; sl < 4; sl++) {
            const float ca = fmaxf(ty0 + (float)(4 * sl), Y - ey), cb = fminf(ty0 + (float)(4 * sl + 4), Y + ey);
            float l = fminf(lo[sl], lo[sl + 1]), h = fmaxf(hi[sl], hi[sl + 1]);
            if ((yl >= ca && yl <= cb) || (yr >= ca && yr <= cb)) { l = fminf(l, X - ex); h = fmaxf(h, X + ex); }
            l -= 0.02f; h += 0.02f;
            unsigned cb4 = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float x0 = tx0 + (float)(4 * c);
                cb4 |= (unsigned)(h >= x0 && l <= x0 + 3.f) << c;
            }
            cols[sl] = col & cb4;
        }
    }
    // block b = 4 * (2 * (cy >> 1) + (cx >> 1)) + 2 * (cy & 1) + (cx & 1)
    unsigned f = 0;
#pragma unroll
    for (int cy = 0; cy < 4; cy++) {
        const unsigned c4 = ((row >> cy) & 1u) ? cols[cy] : 0u;
        f |= (c4 & 3u) << (8 * (cy >> 1) + 2 * (cy & 1));
        f |= (c4 >> 2) << (8 * (cy >> 1) + 4 + 2 * (cy & 1));
    }
    return f;
}
// the exponent of a Gaussian at a pixel, -1/2 (A dx^2 + C dy^2) - B dx dy, with the fused multiply-adds written out ((A, C) and (dx, dy) as register pairs)
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float blend_power(v2f ac, float B, v2f d) {
    const v2f p = ac * d;                                  // (A dx, C dy)
    const float t2 = fmaf(p.y, d.y, p.x * d.x);
    return fmaf(-0.5f, t2, -((B * d.x) * d.y));
}
// expf without the library routine's two range guards: the library's value wherever the result is a normal number
__device__ __forceinline__ float exp_blend(float x) {
    const float ph = x * 0x1.715476p+0f;
    float pl = fmaf(x, 0x1.715476p+0f, -ph);
    pl = fmaf(x, 0x1.4ae0bep-26f, pl);
    const float e = __builtin_rintf(ph);
    const float a = (ph - e) + pl;
    return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
}
// One staged batch: thread t read entry t's 64-byte record.  LT = what a block list holds per entry: uint8_t = the batch index j, uint16_t = 16 j.
template <typename LT>
struct StageLdsT {
    float4 a[BATCH];      // X, Y, r, g
    float4 b[BATCH];      // A, C, B, o
    float4 c[BATCH];      // b, z, -, -
    uint16_t flags[BATCH];
    __attribute__((aligned(16))) LT list[N_BLOCKS][BATCH];
};
template <bool AUX, typename LT>
__device__ __forceinline__ unsigned stage_entry(StageLdsT<LT>& st, const float4* __restrict__ splat, int id, float tx0, float ty0) {
    const float4* rec = splat + 4 * (size_t)id;
    const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
    const unsigned flags = block_flags(q0, q1, q2, tx0, ty0);
    if (flags) {
        st.a[threadIdx.x] = make_float4(q0.x, q0.y, q3.x, q3.y);
        st.b[threadIdx.x] = make_float4(q0.z, q1.x, q0.w, q1.y);
        if constexpr (AUX) *reinterpret_cast<float2*>(&st.c[threadIdx.x]) = make_float2(q3.z, q3.w);
        else st.c[threadIdx.x].x = q3.z;
    }
    return flags;
}
// Builds the 16 per-block lists of a staged batch (ascending batch indices).  Returns the length of the calling thread's own list; *n_wave = the longest
// of the calling wave's four lists.  Contains two barriers: every thread of the workgroup calls it.
template <typename LT>
__device__ __forceinline__ int block_lists(StageLdsT<LT>& st, unsigned flags, int* n_wave) {
    st.flags[threadIdx.x] = (uint16_t)flags;
    __syncthreads();
    const int b = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const uint4 fa = reinterpret_cast<const uint4*>(st.flags)[2 * l16], fb = reinterpret_cast<const uint4*>(st.flags)[2 * l16 + 1];
    const uint32_t w[8] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w};
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t t = (w[k] >> b) & 0x00010001u;
        mask |= ((t & 1u) | (t >> 15)) << (2 * k);
    }
    const int cnt = __popc(mask);
    int incl = cnt;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);  // row_shr:1, zero fill
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, true);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, true);
    const int mine = __shfl(incl, 15, 16);
    LT* dst = st.list[b] + (incl - cnt);
    uint32_t m = mask;
    while (m) {
        const int i = __builtin_ctz(m);
        m &= m - 1u;
        *dst++ = (LT)((16 * l16 + i) * (sizeof(LT) == 2 ? 16 : 1));
    }
    *n_wave = max(max(__builtin_amdgcn_readlane(mine, 0), __builtin_amdgcn_readlane(mine, 16)),
                  max(__builtin_amdgcn_readlane(mine, 32), __builtin_amdgcn_readlane(mine, 48)));
    __syncthreads();
    return mine;
}
// a + (b of the partner lane); CTRL: row_mirror 0x140 (lane ^ 15), row_half_mirror 0x141 (^ 7), quad_perm [3,2,1,0] 0x1b (^ 3), [1,0,3,2] 0xb1 (^ 1)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float keep, float send) {
    return keep + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), CTRL, 0xf, 0xf, true));
}

}  // namespace
