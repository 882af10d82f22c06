// nerf_net.h -- what the forward (nerf_net.hip) and the backward (nerf_grad.hip) of the vanilla NeRF block share: the configuration, the packed
// layout of a weight stream, the streamed GEMM of one weight part (gemm_part), the accumulator -> operand conversion, and the private layout of the
// training workspace (header group 18).  The arithmetic contracts are at the top of the two .hip files.
#pragma once
#include "ngp_net.h"

#define NRC_NERF_TILE_ROWS 128
#define NRC_NERF_MAX_PARTS 24
#define NRC_NERF_MAX_LINEARS 14
#define NRC_NERF_MAX_BIAS 2816   // floats: 8 x 256 + 32 (density) + 256 (feature) + 3 x 128 (colour) + 32 (rgb) + slack, padded to 32 per tile
#define NRC_NERF_SLAB 2048   // uint4 per LDS buffer (32 KB)
#define NRC_NERF_SLAB_TILES (NRC_NERF_SLAB / 64)   // (k-step, m-tile) fragments per slab
#define NRC_NERF_PF (NRC_NERF_SLAB / 256)          // 16-byte loads per thread and slab
#define NRC_NERF_WS_HEADER 16                      // uint4 in front of the training workspace's stages (NerfWs)
#define NRC_NERF_WGRAD_CHUNK_ROWS 2048             // rows per partial sum of the weight gradient

namespace {

struct NerfCfg { int32_t width, n_layers, n_color_layers, n_freq_pos, n_freq_dir, append_input, skip_mask; };

struct NerfPart {
    uint32_t off;       // first uint4 of the part in the blob
    uint32_t first;     // uint4 in its first slab
    int16_t nmt, nks;   // m-tiles (32 output neurons each), k-steps (16 inputs each)
    int16_t src;        // index of the weight in the parameter list
    int16_t natural;    // 1: k in NATURAL order (encodings), 0: ACC order (converted accumulators)
    int32_t rows, ld, col_off, kvalid;
};
struct NerfLinear { uint32_t off; int32_t rows, nmt, src; };   // bias block: off in floats behind bias_base, nmt x 2 x 16 floats in accumulator order
struct NerfLayout {
    int32_t n_parts, n_linears;
    uint32_t w_total;      // uint4 in the weight region
    uint32_t b_total;      // floats in the bias region (behind the weights)
    NerfPart part[NRC_NERF_MAX_PARTS + 1];   // [n_parts]: off = w_total, first = 0
    NerfLinear lin[NRC_NERF_MAX_LINEARS];
};

inline int enc_width(int n_freq, int append) { return 3 * 2 * n_freq + (append ? 3 : 0); }

inline bool cfg_supported(const NerfCfg& c) {
    if (c.width != 128 && c.width != 256) return false;
    if (c.n_layers < 1 || c.n_layers > 8 || c.n_color_layers < 1 || c.n_color_layers > 3) return false;
    if (c.n_freq_pos < 0 || c.n_freq_pos > 10 || c.n_freq_dir < 0 || c.n_freq_dir > 4) return false;
    if (c.append_input != 0 && c.append_input != 1) return false;
    const int np = enc_width(c.n_freq_pos, c.append_input), nd = enc_width(c.n_freq_dir, c.append_input);
    if (np < 1 || np > 64 || nd < 1 || nd > 32) return false;
    // bit k: the encoded position re-enters in front of layer k (0-based), 1 <= k <= n_layers - 1; the module is ill-formed for k = n_layers
    if (c.skip_mask < 0 || (c.skip_mask & ~((1 << c.n_layers) - 2)) != 0) return false;
    return true;
}

// training (group 18): one colour layer, the shape of the reference's configuration; a deeper colour head trains on torch
inline bool train_cfg_supported(const NerfCfg& c) { return cfg_supported(c) && c.n_color_layers == 1; }

// one part of a weight stream behind `off` (which it advances): the first slab is what gemm_part expects to find staged on entry
inline NerfPart make_part(uint32_t& off, int nmt, int nks, int src, int natural, int rows, int ld, int col_off, int kvalid) {
    const int sk = nks < NRC_NERF_SLAB_TILES / nmt ? nks : NRC_NERF_SLAB_TILES / nmt;
    const NerfPart p{off, (uint32_t)(sk * nmt * 64), (int16_t)nmt, (int16_t)nks, (int16_t)src, (int16_t)natural, rows, ld, col_off, kvalid};
    off += (uint32_t)(nmt * nks * 64);
    return p;
}
// the end of a stream: part[n] and everything behind it has off = the stream's size and an empty first slab
inline void close_layout(NerfLayout& L, int n, int nl, uint32_t off, uint32_t boff) {
    L.n_parts = n; L.n_linears = nl; L.w_total = off; L.b_total = boff;
    L.part[n] = NerfPart{off, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = n + 1; k <= NRC_NERF_MAX_PARTS; k++) L.part[k] = L.part[n];
    for (int k = nl; k < NRC_NERF_MAX_LINEARS; k++) L.lin[k] = NerfLinear{0, 0, 0, 0};
}

struct NerfParams { const float* p[2 * NRC_NERF_MAX_LINEARS]; };

__device__ __forceinline__ _Float16 to_h_sat(float v) {
    const _Float16 lim = (_Float16)65504.f;
    _Float16 h = (_Float16)v;
    h = h > lim ? lim : h;
    return h < -lim ? -lim : h;
}

// shared by the forward's encoding and its derivative (nerf_input_grad.hip): sin and cos of an f32 argument, |error| <= 2^-22 for |a| <= 4096 (the contract at the top of nerf_net.hip; tests/nerf_mlp_ref.py restates the sequence)
__device__ __forceinline__ void nerf_sincos(float a, float& sn, float& cs) {
    const float n = rintf(__fmul_rn(a, 0.636619772f));
    float r = fmaf(-n, 1.5703125f, a);
    r = fmaf(-n, 4.837512969970703125e-4f, r);
    r = fmaf(-n, 7.54978995489188216e-8f, r);
    const float z = __fmul_rn(r, r);
    const float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float s = fmaf(__fmul_rn(ps, z), r, r);
    const float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float c = fmaf(pc, __fmul_rn(z, z), fmaf(-0.5f, z, 1.0f));
    const int q = (int)n & 3;
    const float s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
    sn = (q & 2) ? -s1 : s1;
    cs = ((q + 1) & 2) ? -c1 : c1;
}

struct Stream {               // the weight stream of one workgroup: which part comes next, which LDS buffer holds its first slab
    const uint4* blob;
    uint4* lds;
    int p, cur;
};

// acc += W_part . B.  NKS k-steps of B, NMT m-tiles; the part's first slab is in buffer st.cur on entry, the next part's first slab on exit.
template <int NMT, int NKS>
__device__ __forceinline__ void gemm_part(f16v (&acc)[NMT], const h8* B, const NerfLayout& L, Stream& st, int tid, int lane) {
    constexpr int SK = NKS < NRC_NERF_SLAB_TILES / NMT ? NKS : NRC_NERF_SLAB_TILES / NMT, NS = NKS / SK, SLAB = SK * NMT * 64;
    static_assert(NKS % SK == 0 && SLAB <= NRC_NERF_SLAB, "slab shape");
    const uint32_t off = L.part[st.p].off, next_off = L.part[st.p + 1].off, next_cnt = L.part[st.p + 1].first;
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const uint4* src = (i + 1 < NS) ? st.blob + off + (i + 1) * SLAB : st.blob + next_off;
        const uint32_t cnt = (i + 1 < NS) ? (uint32_t)SLAB : next_cnt;
        uint4 pf[NRC_NERF_PF];
#pragma unroll
        for (int q = 0; q < NRC_NERF_PF; q++) {
            const uint32_t e = (uint32_t)tid + 256u * q;
            pf[q] = make_uint4(0u, 0u, 0u, 0u);
            if (e < cnt) pf[q] = src[e];
        }
        // the slab's SK x NMT fragments in the order of use, DEPTH reads ahead of the MFMA that consumes them: with one wave per SIMD nothing else
        // hides the LDS latency (two reads in flight, the compiler's own schedule, left the matrix pipe idle three clocks out of four)
        const uint4* buf = st.lds + st.cur * NRC_NERF_SLAB + lane;
        constexpr int NT = SK * NMT, WANT = NMT < 8 ? 4 : 8, DEPTH = NT < WANT ? NT : WANT;   // (eight at W = 128 would cost that width its second wave per SIMD)
        uint4 ring[DEPTH];
#pragma unroll
        for (int t = 0; t < DEPTH; t++) ring[t] = buf[t * 64];
        __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise sinks every read back to its use)
#pragma unroll
        for (int t = 0; t < NT; t++) {
            acc[t % NMT] = NRC_MFMA(*reinterpret_cast<const h8*>(&ring[t % DEPTH]), B[i * SK + t / NMT], acc[t % NMT]);
            if (t + DEPTH < NT) ring[t % DEPTH] = buf[(t + DEPTH) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
        uint4* nb = st.lds + (st.cur ^ 1) * NRC_NERF_SLAB;
#pragma unroll
        for (int q = 0; q < NRC_NERF_PF; q++) {
            const uint32_t e = (uint32_t)tid + 256u * q;
            if (e < cnt) nb[e] = pf[q];
        }
        __syncthreads();
        st.cur ^= 1;
    }
    st.p++;
}

// accumulator -> next operand: fp16 (RNE), then ReLU (optional), then saturation, the last two packed
template <bool RELU>
__device__ __forceinline__ h8 to_operand(const f16v& acc, int g) {
    h8 f;
#pragma unroll
    for (int j = 0; j < 8; j++) f[j] = (_Float16)acc[8 * g + j];
    const _Float16 m = (_Float16)65504.f, lo = RELU ? (_Float16)0.f : -m;
    const h8 vlo = {lo, lo, lo, lo, lo, lo, lo, lo}, vhi = {m, m, m, m, m, m, m, m};
    return __builtin_elementwise_min(__builtin_elementwise_max(f, vlo), vhi);
}
template <int NMT, bool RELU>
__device__ __forceinline__ void to_operands(const f16v (&acc)[NMT], h8* H) {
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) { H[2 * mt] = to_operand<RELU>(acc[mt], 0); H[2 * mt + 1] = to_operand<RELU>(acc[mt], 1); }
}

// ---- the training workspace (group 18; private) -------------------------------------------------------------------------------------------------
// [header: NRC_NERF_WS_HEADER uint4][saved operands][pre-activation gradients][f32 partial sums of the weight gradient].  Rows are padded to whole
// workgroup tiles (128).  A stage of `nks` k-steps (16 columns each) is stored as the fragments its producer holds: uint4 (tile32 * nks + s) * 64 + lane
// behind the stage's base, tile32 = row / 32, lane = 32 hh + row % 32, the eight fp16 = columns 16 s + 8 hh + j of the stage in FRAGMENT order
// (NATURAL stages: the column is the feature; ACC stages: feature = the column with bits 2 and 3 exchanged -- frag_col).  A wave stores or loads
// 1 KB of consecutive bytes per fragment; the weight-gradient kernel, which needs the ROWS of a column side by side, transposes through LDS.
// Header (int32): [0] bits of max |head gradient| at scale 1 (automatic scale), [1] saturated gradient elements, [2..3] reserved.
// Saved stages t = 0 ..: enc_pos (4 k-steps), enc_dir (2), H_1 .. H_L (W / 16), F (W / 16), C_1 (W / 32) -- tap t + 1 of the forward.
// Gradient stages g = 0 ..: rgb head (1 k-step, 3 columns), C_1, F, sigma head (1 k-step, 1 column), H_L .. H_1 -- the order of the backward.
struct NerfWs {
    int64_t tiles32;       // 32-row tiles (a multiple of 4)
    int32_t nk, L;
    __host__ __device__ int saved_nks(int t) const { return t == 0 ? 4 : (t == 1 ? 2 : (t == L + 3 ? nk / 2 : nk)); }
    __host__ __device__ int saved_ks(int t) const { return t == 0 ? 0 : (t == 1 ? 4 : 6 + (t - 2) * nk); }          // k-steps in front of saved stage t
    __host__ __device__ int saved_total() const { return 6 + (L + 1) * nk + nk / 2; }
    __host__ __device__ int grad_nks(int g) const { return (g == 0 || g == 3) ? 1 : (g == 1 ? nk / 2 : nk); }
    __host__ __device__ int grad_ks(int g) const {                                                                     // ... in front of gradient stage g
        return saved_total() + (g == 0 ? 0 : (g == 1 ? 1 : (g == 2 ? 1 + nk / 2 : (g == 3 ? 1 + nk / 2 + nk : 2 + nk / 2 + nk + (g - 4) * nk))));
    }
    __host__ __device__ int total_ks() const { return saved_total() + 2 + nk / 2 + nk + L * nk; }
    __host__ __device__ int64_t stage_base(int ks) const { return NRC_NERF_WS_HEADER + tiles32 * 64 * (int64_t)ks; }   // uint4 index
    __host__ __device__ int64_t partial_base() const { return stage_base(total_ks()); }                                // uint4 index of the f32 partial sums
};
inline NerfWs make_ws(const NerfCfg& c, int64_t M) {
    return NerfWs{nrc_cdiv(M, NRC_NERF_TILE_ROWS) * (NRC_NERF_TILE_ROWS / 32), c.width / 16, c.n_layers};
}
__host__ __device__ __forceinline__ int frag_col(int feature, int natural) {   // column of a feature in a stage (its own inverse)
    return natural ? feature : ((feature & ~12) | ((feature & 4) << 1) | ((feature & 8) >> 1));
}

}  // namespace
