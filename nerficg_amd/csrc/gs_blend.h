// gs_blend.h -- what the blend-family kernels share: k_render / k_render_bw (gs_raster.hip), k_render_features / k_render_features_bw (gs_features.hip) and
// k_gs_contributions (gs_contrib.hip).  The ONE definition of the pixel layout of a tile, the conservative per-block test, the exponent, the exponential, the
// staged batch and its sixteen per-block work lists, the forward replay of a staged batch, the DPP exchange-and-add, and (host) the band rule and the check of
// the state a colour forward leaves behind.  The three translation units are built with the same flags (build.py: GS_BLEND_FLAGS), so a kernel that replays
// the blend with these statements computes alpha -- hence the blended set and every weight alpha T -- bit for bit as the colour pass does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TILE 16
#define BATCH 256
#define N_BLOCKS 16
// The blend backward's per-Gaussian accumulator: ONE 64-byte record per Gaussian,
//   [0..2] dL/dcolour   [3] dL/dopacity   [4..5] dL/dmean2D (x, y)   [6..8] dL/dconic (xx, xy, yy)   [9] dL/dz (depth-and-alpha backward)   [10..15] unused,
// so that the nine sums a tile flushes for a Gaussian are one contiguous 36-byte group of ONE atomic wave-instruction.  Round 2 kept them in four
// arrays (colour (P,3), opacity (P), mean2D (P,3), conic (P,4)): nine atomic instructions per flushing thread, every lane of each in another
// cache line -- float atomics execute at the memory side, per 64-byte request, and that shape is the slow one (MI355X_MICROARCH.md, Global float
// atomics: "64 lanes in 64 different rows ~17x slower").  Ablation (round 3): without the flush k_render_bw took 367 instead of 485 us.
#define GREC 16

namespace {

// thread -> pixel of the 16x16 tile: wave = 8x8 quadrant, DPP row (16 lanes) = 4x4 block of the quadrant.  block index b = 4 * wave + row,
// block (cx, cy) of the 4x4 block grid of the tile: cx = 2 * (wave & 1) + (row & 1), cy = 2 * (wave >> 1) + (row >> 1).
__device__ __forceinline__ int tile_px(unsigned t) { return (int)((t & 3u) + ((t >> 4) & 1u) * 4u + ((t >> 6) & 1u) * 8u); }
__device__ __forceinline__ int tile_py(unsigned t) { return (int)(((t >> 2) & 3u) + ((t >> 5) & 1u) * 4u + (t >> 7) * 8u); }
// what a thread of a forward-walking kernel knows of its tile (of a frame gx tiles wide) and its pixel.  (The two backward kernels state the same quantities
// themselves, in another order: with these statements their machine code moves, k_render's and the replaying kernels' does not -- LABBOOK.)
struct TilePixel {
    int tile_x, tile_y, px, py;
    bool inside;       // the pixel lies in the W x H image (partial tiles at the right and bottom edges)
    float fx, fy;      // the pixel centre the splat records measure from
    float tx0, ty0;    // the tile's first pixel
    int block;         // = 4 * wave + DPP row
    __device__ __forceinline__ TilePixel(int tile, int gx, int W, int H)
        : tile_x(tile % gx), tile_y(tile / gx), px(tile_x * TILE + tile_px(threadIdx.x)), py(tile_y * TILE + tile_py(threadIdx.x)), inside(px < W && py < H),
          fx((float)px), fy((float)py), tx0((float)(tile_x * TILE)), ty0((float)(tile_y * TILE)), block(threadIdx.x >> 4) {}
};
// The tile lists come from the square 3-sigma bound of preprocess (reference semantics, kept bit-exact), but a pixel only blends a
// Gaussian where alpha = o exp(power) >= 1/255, i.e. inside the ellipse A dx^2 + 2 B dx dy + C dy^2 <= 2 ln(255 o).  On the bench
// scene 52 % of the (tile, Gaussian) pairs of a list have no such pixel in the tile, and the box of a pair that has is ~5 pixels wide
// (tools/gs_stats.py): it reaches 2.5 of the four 8x8 quadrants (160 lanes) but only ~5 of the sixteen 4x4 blocks (80 lanes).
// Both render kernels therefore keep ONE WORK LIST PER 4x4 BLOCK: while a batch of 256 list entries is staged into LDS every thread tests
// its entry's box against the 16 blocks; 16 ballots and a prefix over the 4 waves turn the flags into 16 ascending index lists; and every
// DPP row of a wave walks ITS OWN list -- the four rows of a wave blend four different Gaussians in the same instruction.  The box is
// conservative (margins below), so exactly the same pixels blend exactly the same Gaussians in the same order: bit-identical pictures.
// bit b set when the alpha >= 1/255 ellipse of the record can reach a pixel centre of block b (block = 4 x 4 pixels of the 16 x 16 tile).
// Two conservative tests: the ellipse's bounding box against the four column / row bands, then, per row band, the x-interval the ellipse
// spans inside the band (chords at the band's two edges -- clamped to the ellipse's y-range --, widened to the box where the leftmost /
// rightmost point of the ellipse lies inside the band) against the column bands.  On the bench scene the box keeps 6.2 blocks per
// (tile, Gaussian) pair of a blended prefix, the band intervals 4.7, an exact per-pixel test 4.5 (tools/gs_stats.py).
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
// The exponent of a Gaussian at a pixel: -1/2 (A dx^2 + C dy^2) - B dx dy, as SIX instructions (one of them packed) with explicit fused multiply-adds where the source-order
// form takes nine (the including translation units are built without contraction: the integer decisions of the per-Gaussian kernels must not move).  The blend
// kernels are bound by VALU issue (profiles/: 0.70-0.78 of the issue slots at 315 M blends per frame), so instructions per blend are what they cost.
// The upstream binary is an nvcc build with -fmad=true, i.e. it fuses in these places too; WHICH pairs it fuses is not recoverable, so the oracle
// (oracle/gs_oracle_impl.h: GS_BLEND_POWER / test_T / the colour sums) states the same fusions and n_contrib / final_T stay bit-exact against it.
typedef float v2f __attribute__((ext_vector_type(2)));
// (A, C) and (dx, dy) travel as register PAIRS: the two first products are one v_pk_mul_f32, the pixel offset one v_pk_add_f32 -- the same
// roundings as the scalar form, two VALU instructions less per blend.  (The including translation units are built with -fno-slp-vectorize: left to itself
// the vectoriser pairs the products of two DIFFERENT list entries and pays the packing back in v_mov, 20 per four blends.)
__device__ __forceinline__ float blend_power(v2f ac, float B, v2f d) {
    const v2f p = ac * d;                                  // (A dx, C dy)
    const float t2 = fmaf(p.y, d.y, p.x * d.x);
    return fmaf(-0.5f, t2, -((B * d.x) * d.y));
}
// expf for the blend loops, WITHOUT the two range guards of the library routine: the same nine instructions (Cody-Waite split of x log2(e), v_exp_f32 on the
// fraction, v_ldexp_f32 by the integer part), hence bit for bit the library's value wherever the result is a normal number, -87.3 <= x <= 88.72
// (tools/micro/exp_blend_check.hip: 2 x 10^8 inputs -- a sweep of [-104, 0], every float in [-1e-3, 0], 2^13 floats around every multiple of ln 2 --
// 0 differences there; below, where the result is a denormal, the two differ in how they flush: a blend needs alpha >= 1/255, i.e. x >= -5.6, so none
// of those values is ever used).  The four instructions dropped -- two compares and two selects forcing 0 / inf outside the range -- were a tenth of
// k_render's VALU instructions per blend (40 -> 36; 168 -> 157 us at 1 M Gaussians).  x > 88.72 (power > 0: the blend discards the entry) overflows to
// inf in v_ldexp_f32 like the library's select.
__device__ __forceinline__ float exp_blend(float x) {
    const float ph = x * 0x1.715476p+0f;
    float pl = fmaf(x, 0x1.715476p+0f, -ph);
    pl = fmaf(x, 0x1.4ae0bep-26f, pl);
    const float e = __builtin_rintf(ph);
    const float a = (ph - e) + pl;
    return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
}
// One staged batch: thread t read entry t's 64-byte record; what the blend loop needs goes to LDS as two 16-byte vectors and a scalar.
// LT = what a block list holds per entry: uint8_t = the batch index j (k_render_bw: its LDS budget, with the 18 KB of per-Gaussian sums, has no
// room for more), uint16_t = 16 j, the BYTE OFFSET of the entry's records in a[] / b[] / c[] (k_render: the address arrives with the list read, three
// VALU instructions per blend less).  Blue sits in a float4 array of its own so that all three records of an entry live at the same offset.
template <typename LT>
struct StageLdsT {
    float4 a[BATCH];      // X, Y, r, g
    float4 b[BATCH];      // A, C, B, o  (conic xx, yy, xy, opacity: the pair (A, C) is what blend_power multiplies with (dx, dy))
    float4 c[BATCH];      // b, z, -, -  (z: staged by the depth-and-alpha instances only)
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
// Builds the 16 per-block lists of a staged batch: the 16 lanes of DPP row b (= the threads whose pixels form block b) build list b, lane l
// from the flags of entries 16 l .. 16 l + 15 (two 16-byte LDS reads), ranked with a row prefix sum.  st.list[b] receives the batch indices
// of the entries that reach block b in ascending order.  Returns the length of the calling thread's own list; *n_wave = the longest of the
// calling wave's four lists.  Contains two barriers: every thread of the workgroup calls it.
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

// ---- the forward walk over a staged batch with byte-offset lists (k_render, and the kernels that replay it: k_render_features, k_gs_contributions) ----
// Everything the blend loop reads from LDS must be FINITE also for a row that is past the end of its list and picks up a stale index (it meets a weight of
// exactly 0): thread t clears slot t of a[] and b[], which only thread t ever stages into.  And every list entry it can pick up must be a valid offset: the lists
// start as zeros too (later batches leave offsets of earlier entries behind).  What else a kernel reads through the offsets (c[] in k_render, the staged
// features in k_render_features) it clears itself, between the two calls.
__device__ __forceinline__ void stage_clear_records(StageLdsT<uint16_t>& st) {
    st.a[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f); st.b[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void stage_clear_lists(StageLdsT<uint16_t>& st) {
    reinterpret_cast<uint4*>(&st.list[0][0])[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    reinterpret_cast<uint4*>(&st.list[0][0])[256 + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}
// one LDS read of a row's list = four entries: off[u] = 16 j.  Entries behind the list end are stale offsets of earlier batches (or zeros): readable, masked by the caller
__device__ __forceinline__ void unpack_offsets(uint2 pack, int (&off)[4]) {
    off[0] = (int)(pack.x & 0xffffu); off[1] = (int)(pack.x >> 16); off[2] = (int)(pack.y & 0xffffu); off[3] = (int)(pack.y >> 16);
}
// The colour pass's alpha of the four entries off[] of a row's list (entries jj .. jj + 3 of n_mine) at pixel (fx, fy), and ok[u]: the colour pass blended entry u
// here -- it is an entry of the list, not behind the pixel's n_contrib (`last`; pos0 = the contributor number of batch entry 0), and passes the two alpha tests.
// The saturation test needs no replay: n_contrib is where it struck.
__device__ __forceinline__ void replay_pack(const StageLdsT<uint16_t>& st, const int (&off)[4], int jj, int n_mine, uint32_t pos0, uint32_t last, float fx, float fy,
                                            float (&alpha)[4], bool (&ok)[4]) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const float4 a_j = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(st.a) + off[u]);
        const float4 b_j = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(st.b) + off[u]);
        const v2f d = (v2f){a_j.x, a_j.y} - (v2f){fx, fy};
        const float power = blend_power((v2f){b_j.x, b_j.y}, b_j.z, d);
        alpha[u] = fminf(0.99f, b_j.w * exp_blend(power));
        ok[u] = (jj + u < n_mine) & (pos0 + ((uint32_t)off[u] >> 4) <= last) & !(power > 0.0f) & !(alpha[u] < 1.0f / 255.0f);
    }
}

// a + (b of the partner lane); CTRL: row_mirror 0x140 (lane ^ 15), row_half_mirror 0x141 (^ 7), quad_perm [3,2,1,0] 0x1b (^ 3), [1,0,3,2] 0xb1 (^ 1)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float keep, float send) {
    return keep + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), CTRL, 0xf, 0xf, true));
}

// ---- host: what every band entry point checks before anything else (no HIP call in front of it) ----
// a band = tile rows [begin, begin + n) of the frame's ceil(H / 16) rows
inline bool gs_band_ok(int32_t H, int32_t tile_row_begin, int32_t n_tile_rows) {
    if (H < 1 || tile_row_begin < 0 || n_tile_rows < 1) return false;
    return (int64_t)tile_row_begin + n_tile_rows <= (int64_t)((H + TILE - 1) / TILE);
}
// the state a colour forward of the band left behind, as the passes that replay it receive it (groups 21 and 22).  P == 0: the lists are empty and nothing reads
// point_list or the splat records (four 16-byte vectors per Gaussian)
inline bool gs_saved_state_ok(int32_t P, int32_t W, int32_t H, const int32_t* point_list, const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order,
                              const uint32_t* n_contrib, int32_t tile_row_begin, int32_t n_tile_rows) {
    if (!gs_band_ok(H, tile_row_begin, n_tile_rows) || P < 0 || W < 1) return false;
    if (!ranges || !tile_order || !n_contrib) return false;
    if (P > 0 && (!point_list || !splat_records)) return false;
    return (reinterpret_cast<uintptr_t>(splat_records) & 15u) == 0;
}

}  // namespace
