// nerf_grad.hip -- the vanilla NeRF block's TRAINING backward (header group 18): the data gradient through the whole block as one kernel on
// v_mfma_f32_32x32x16_f16, the weight and bias gradients as one kernel per (row chunk, output block) plus a fixed-order reduction.  The training
// forward is the third instantiation of k_nerf_forward (nerf_net.hip); the workspace layout both sides share is NerfWs (nerf_net.h).
//
// ARITHMETIC CONTRACT (restated in f64 by tests/nerf_grad_ref.py).  S = 2^e is the scale, X_l the saved fp16 operand entering linear l,
// W16 the fp16 weights of the blob (the same values as the forward's: round-to-nearest-even, clamped at +-65504).
//   * heads, f32:  g_rgb = (d_rgb S) (rgb (1 - rgb))  -- three roundings: 1 - rgb, its product with rgb, the product with the exactly scaled d_rgb;
//     g_sigma = d_sigma S where the forward's sigma > 0, else 0.  Both are then converted to fp16 (RNE) and saturated at +-65504.
//   * data gradient of a linear:  dX[m, i] = sum_o W16[o, i] G[m, o], fp16 operands, ONE f32 accumulator starting at 0 for all consumers of a stage
//     (H_L feeds the density head and the feature layer) in the order of the matrix instruction; then G_prev = sat(fp16(dX)) where the saved operand
//     X > 0 (a saturated operand passes the gradient), 0 elsewhere.  The feature stage F has no ReLU and no mask.  The encoded position and direction
//     receive no gradient: the skip columns and the colour layer's direction columns are not propagated.
//   * weights and biases:  dW[o, i] = (sum_m G[m, o] X_l[m, i]) / S,  db[o] = (sum_m G[m, o]) / S.  Products of fp16 values, f32 accumulation.  The order is
//     fixed: inside a chunk of NRC_NERF_WGRAD_CHUNK_ROWS rows the order of the matrix instruction over ascending 16-row steps (the bias: eight rows per
//     lane, ascending, then the two lane halves), then the chunks in ascending order, then one multiplication by 2^-e (exact unless the result is
//     subnormal).  No floating-point atomics: two calls give the same bits.  Straight-through with respect to the f32 master weights.
//   * rows: G[m, .] depends on row m and the weights only; padded rows have zero head gradients, hence G = 0, and their saved operands are finite
//     (the forward's clamped copy of the last row): they add exactly 0 to dW and db.
//   * scale: automatic -- e = 12 - floor(log2 max |head gradient at S = 1|), the maximum by an integer atomicMax on the bit patterns (deterministic);
//     a zero or non-finite maximum gives e = 0; e is clamped to +-126.  A caller's grad_scale (a positive power of two) replaces it.
//     Gradient elements whose fp16 conversion overflowed (|f32 value| >= 65520) and was saturated at +-65504 are counted (stats[1]).
#include "nerf_net.h"

#define NRC_NERF_WG_LD 40        // halves per LDS column of the weight-gradient tile: 32 rows + 8 of padding (16-byte aligned fragments)
#define NRC_NERF_WG_COLS 448     // 320 operand columns (W + 64 at most) + 128 gradient columns
#define NRC_NERF_WG_NT 10        // 32-column tiles of the operand at most
#define NRC_NERF_WG_PF 7         // 16-byte loads per thread and 32-row tile at most (448 / 16 fragments x 64 lanes / 256 threads)
#define NRC_NERF_MAX_UNITS 24

namespace {

// ---- the transposed weight stream ---------------------------------------------------------------------------------------------------------------
// The parts of the data gradient in the order the kernel consumes them; A[row = input i][k = output o] = W16[o, i].
void make_layout_t(const NerfCfg& c, NerfLayout& L) {
    const int W = c.width, NM = W / 32, NK = W / 16, np = enc_width(c.n_freq_pos, c.append_input), nd = enc_width(c.n_freq_dir, c.append_input);
    const int Ln = c.n_layers;
    int n = 0;
    uint32_t off = 0;
    auto part = [&](int nmt, int nks, int lin, int natural, int rows, int ld, int kvalid) {
        L.part[n++] = make_part(off, nmt, nks, 2 * lin, natural, rows, ld, 0, kvalid);
    };
    part(NM / 2, 1, Ln + 3, 1, W / 2, W / 2, 3);          // rgb head: C_1 <- g_rgb
    part(NM, NK / 2, Ln + 2, 0, W, W + nd, W / 2);        // colour layer: F <- G(C_1), feature columns only
    part(NM, NK, Ln + 1, 0, W, W, W);                     // feature layer: H_L <- G(F)
    part(NM, 1, Ln, 1, W, W, 1);                          // density head: H_L <- g_sigma, same accumulator
    for (int l = Ln - 1; l >= 1; l--) part(NM, NK, l, 0, W, W + (((c.skip_mask >> l) & 1) ? np : 0), W);   // H_l <- G(H_l+1), hidden columns only
    close_layout(L, n, 0, off, 0);
}

__global__ void __launch_bounds__(256) k_nerf_pack_t(NerfParams P, NerfLayout L, uint4* __restrict__ blob) {
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
        const int k = q.natural ? 16 * s + 8 * hh + j : 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3);
        f[j] = (row < q.rows && k < q.kvalid) ? to_h_sat(src[(size_t)k * q.ld + row]) : (_Float16)0.f;
    }
    blob[idx] = *reinterpret_cast<const uint4*>(&f);
}

// ---- scale ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int scale_exponent(const int32_t* hdr, int fixed, int fixed_exp) {
    if (fixed) return fixed_exp;
    const uint32_t bits = (uint32_t)hdr[0];
    if (bits == 0u || bits >= 0x7f800000u) return 0;
    const int ex = (int)(bits >> 23);
    const int fl = ex > 0 ? ex - 127 : (31 - __clz((int)bits)) - 149;   // floor(log2 max), subnormals included
    const int e = 12 - fl;
    return e > 126 ? 126 : (e < -126 ? -126 : e);
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }   // -126 <= e <= 127

__device__ __forceinline__ float rgb_slope(float r) { return __fmul_rn(r, __fsub_rn(1.f, r)); }

__global__ void __launch_bounds__(256) k_nerf_head_max(const float* __restrict__ d_sigma, const float* __restrict__ d_rgb, const float* __restrict__ sigma,
                                                       const float* __restrict__ rgb, int64_t M, int32_t* __restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t m = 0u;
    if (i < M) {
        m = __float_as_uint(fabsf(sigma[i] > 0.f ? d_sigma[i] : 0.f));
#pragma unroll
        for (int ch = 0; ch < 3; ch++) m = max(m, __float_as_uint(fabsf(__fmul_rn(d_rgb[3 * i + ch], rgb_slope(rgb[3 * i + ch])))));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(reinterpret_cast<uint32_t*>(hdr), m);
}

// ---- data gradient -------------------------------------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void load_stage(h8* F, const uint4* ws, int64_t base, int64_t tile32, int lane) {
    const uint4* src = ws + base + tile32 * N * 64 + lane;
#pragma unroll
    for (int s = 0; s < N; s++) { const uint4 v = src[s * 64]; F[s] = *reinterpret_cast<const h8*>(&v); }
}
template <int N>
__device__ __forceinline__ void store_stage(const h8* F, uint4* ws, int64_t base, int64_t tile32, int lane) {
    uint4* dst = ws + base + tile32 * N * 64 + lane;
#pragma unroll
    for (int s = 0; s < N; s++) dst[s * 64] = *reinterpret_cast<const uint4*>(&F[s]);
}
template <int NMT>
__device__ __forceinline__ void zero_acc(f16v (&acc)[NMT]) {
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) acc[mt] = zero16();
}

// the f32 tile -> the pre-activation gradient of the stage: sat(fp16(dX)) where the saved operand X is > 0 (MASK), 0 elsewhere; X holds the saved
// fragments on entry and the gradient on exit.  On packed halves, as integer words: a half is kept when its sign is clear and its magnitude is not
// zero; a kept half that the saturation changed (inf ^ 65504 = 0x07ff: bit 0) is counted in nsat, one population count per fragment.  (Counting on
// the f32 values, or element by element, kept copies of the accumulators in vector registers: 96 - 120 bytes of scratch per lane at W = 256.)
template <int NMT, bool MASK>
__device__ __forceinline__ void to_gradient(const f16v (&acc)[NMT], h8* X, int& nsat) {
#pragma unroll
    for (int mt = 0; mt < NMT; mt++)
#pragma unroll
        for (int g = 0; g < 2; g++) {
            h8 f;
#pragma unroll
            for (int j = 0; j < 8; j++) f[j] = (_Float16)acc[mt][8 * g + j];
            const h8 v = to_operand<false>(acc[mt], g);
            const uint4 fw = *reinterpret_cast<const uint4*>(&f), vw = *reinterpret_cast<const uint4*>(&v), xw = *reinterpret_cast<const uint4*>(&X[2 * mt + g]);
            const uint32_t fa[4] = {fw.x, fw.y, fw.z, fw.w}, va[4] = {vw.x, vw.y, vw.z, vw.w}, xa[4] = {xw.x, xw.y, xw.z, xw.w};
            uint32_t o[4], satw[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t keep = 0xffffffffu;
                if constexpr (MASK) keep = (((((xa[q] & 0x7fff7fffu) + 0x7fff7fffu) & ~xa[q]) & 0x80008000u) >> 15) * 0xffffu;
                o[q] = va[q] & keep;
                satw[q] = (fa[q] ^ va[q]) & keep & 0x00010001u;
            }
            nsat += __popc(satw[0] | (satw[1] << 1) | (satw[2] << 2) | (satw[3] << 3));
            const uint4 ow = make_uint4(o[0], o[1], o[2], o[3]);
            X[2 * mt + g] = *reinterpret_cast<const h8*>(&ow);
        }
}

template <int W>
__global__ void __launch_bounds__(256) k_nerf_dgrad(const float* __restrict__ d_sigma, const float* __restrict__ d_rgb, const float* __restrict__ sigma,
                                                    const float* __restrict__ rgb, int64_t M, const uint4* __restrict__ blob_t, NerfCfg c, NerfLayout L,
                                                    uint4* __restrict__ ws, int fixed, int fixed_exp) {
    constexpr int NM = W / 32, NK = W / 16;
    __shared__ uint4 lds[2 * NRC_NERF_SLAB];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int64_t i = (int64_t)blockIdx.x * NRC_NERF_TILE_ROWS + (tid >> 6) * 32 + r;
    const int64_t tile32 = (int64_t)blockIdx.x * (NRC_NERF_TILE_ROWS / 32) + (tid >> 6);
    const NerfWs S{(int64_t)gridDim.x * (NRC_NERF_TILE_ROWS / 32), NK, c.n_layers};
    int32_t* hdr = reinterpret_cast<int32_t*>(ws);
    const float scale = pow2f(scale_exponent(hdr, fixed, fixed_exp));

    Stream st{blob_t, lds, 0, 0};
#pragma unroll
    for (int q = 0; q < NRC_NERF_PF; q++) {
        const uint32_t e = (uint32_t)tid + 256u * q;
        if (e < L.part[0].first) lds[e] = blob_t[e];
    }

    // head gradients as NATURAL-order fragments of one k-step: column ch of g_rgb, column 0 of g_sigma, on lane half 0; zero for padded rows
    int nsat = 0;
    h8 g_rgb, g_sig;
#pragma unroll
    for (int j = 0; j < 8; j++) { g_rgb[j] = (_Float16)0.f; g_sig[j] = (_Float16)0.f; }
    if (i < M && hh == 0) {
        const float gs = sigma[i] > 0.f ? __fmul_rn(d_sigma[i], scale) : 0.f;
        nsat += fabsf(gs) >= 65520.f ? 1 : 0;
        g_sig[0] = to_h_sat(gs);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float g = __fmul_rn(__fmul_rn(d_rgb[3 * i + ch], scale), rgb_slope(rgb[3 * i + ch]));
            asm volatile("" : "+v"(g));   // the f32 product, THEN the conversion: left alone the compiler fuses the two into one v_fma_mixlo_f16, which rounds once
            nsat += fabsf(g) >= 65520.f ? 1 : 0;
            g_rgb[ch] = to_h_sat(g);
        }
    }
    store_stage<1>(&g_rgb, ws, S.stage_base(S.grad_ks(0)), tile32, lane);
    store_stage<1>(&g_sig, ws, S.stage_base(S.grad_ks(3)), tile32, lane);
    __syncthreads();

    h8 G[NK];
    {   // rgb head -> C_1 (masked) -> F (no mask)
        f16v ac[NM / 2];
        h8 C[NK / 2];
        load_stage<NK / 2>(C, ws, S.stage_base(S.saved_ks(c.n_layers + 3)), tile32, lane);
        zero_acc<NM / 2>(ac);
        gemm_part<NM / 2, 1>(ac, &g_rgb, L, st, tid, lane);
        to_gradient<NM / 2, true>(ac, C, nsat);
        store_stage<NK / 2>(C, ws, S.stage_base(S.grad_ks(1)), tile32, lane);
        f16v acc[NM];
        zero_acc<NM>(acc);
        gemm_part<NM, NK / 2>(acc, C, L, st, tid, lane);
        to_gradient<NM, false>(acc, G, nsat);
        store_stage<NK>(G, ws, S.stage_base(S.grad_ks(2)), tile32, lane);
    }
    f16v acc[NM];
    h8 X[NK];
    // H_L: the feature layer and the density head in one accumulator
    load_stage<NK>(X, ws, S.stage_base(S.saved_ks(c.n_layers + 1)), tile32, lane);
    zero_acc<NM>(acc);
    gemm_part<NM, NK>(acc, G, L, st, tid, lane);
    gemm_part<NM, 1>(acc, &g_sig, L, st, tid, lane);
    to_gradient<NM, true>(acc, X, nsat);
    store_stage<NK>(X, ws, S.stage_base(S.grad_ks(4)), tile32, lane);
    for (int l = c.n_layers - 1; l >= 1; l--) {   // H_l from G(H_l+1) through the hidden columns of layer l
#pragma unroll
        for (int s = 0; s < NK; s++) G[s] = X[s];
        load_stage<NK>(X, ws, S.stage_base(S.saved_ks(l + 1)), tile32, lane);
        zero_acc<NM>(acc);
        gemm_part<NM, NK>(acc, G, L, st, tid, lane);
        to_gradient<NM, true>(acc, X, nsat);
        store_stage<NK>(X, ws, S.stage_base(S.grad_ks(4 + c.n_layers - l)), tile32, lane);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nsat += __shfl_xor(nsat, d);
    if (lane == 0 && nsat) atomicAdd(&hdr[1], nsat);
}

// ---- weight and bias gradient --------------------------------------------------------------------------------------------------------------------
// One unit = one linear's output block of <= 128 gradient columns against ALL its operand columns ([hidden | encoded position], [F | encoded direction]).
struct WUnit {
    int32_t g_ks, g_stage_nks, g_s0, g_nks;   // gradient stage: k-steps in front of it, its k-steps per tile, this block's first k-step and k-steps
    int32_t x_ks[2], x_nks[2];                // operand stages (whole): k-steps in front, k-steps per tile (0: none)
    uint32_t poff;                            // floats in front of the unit in a chunk's partial sums: [16 g_nks][16 (x_nks0 + x_nks1)] then [16 g_nks] bias
};
struct WLin {
    int32_t rows, ld;          // the weight: (rows, ld) row-major
    int32_t xw[2], xnat[2];    // operand widths (features) and orders
    int32_t gnat, unit0;       // order of the gradient stage, first unit
    uint32_t off;              // floats in front of the weight in grad_params; the bias follows the weight
};
struct WPlan {
    int32_t n_units, n_lin;
    uint32_t chunk_floats, total;   // floats per chunk of partial sums; floats in grad_params
    WUnit u[NRC_NERF_MAX_UNITS];
    WLin lin[NRC_NERF_MAX_LINEARS];
};

void make_plan(const NerfCfg& c, const NerfWs& S, WPlan& P) {
    const int W = c.width, Ln = c.n_layers, np = enc_width(c.n_freq_pos, c.append_input), nd = enc_width(c.n_freq_dir, c.append_input);
    int nu = 0, nl = 0;
    uint32_t poff = 0, off = 0;
    // g: gradient stage; x0 / x1: saved stages (-1: none) with their valid widths
    auto linear = [&](int g, int gnat, int rows, int x0, int x0w, int x0nat, int x1, int x1w) {
        P.lin[nl++] = WLin{rows, x0w + x1w, {x0w, x1w}, {x0nat, 1}, gnat, nu, off};
        off += (uint32_t)(rows * (x0w + x1w) + rows);
        const int gn = S.grad_nks(g);
        for (int s0 = 0; s0 < gn; s0 += 8) {
            const int n = gn - s0 < 8 ? gn - s0 : 8, xn0 = S.saved_nks(x0), xn1 = x1 >= 0 ? S.saved_nks(x1) : 0;
            P.u[nu++] = WUnit{S.grad_ks(g), gn, s0, n, {S.saved_ks(x0), x1 >= 0 ? S.saved_ks(x1) : 0}, {xn0, xn1}, poff};
            poff += (uint32_t)(16 * n * 16 * (xn0 + xn1) + 16 * n);
        }
    };
    linear(3 + Ln, 0, W, 0, np, 1, -1, 0);                                                                  // layer 0: enc_pos -> H_1
    for (int l = 1; l < Ln; l++) {
        const int skip = (c.skip_mask >> l) & 1;
        linear(3 + Ln - l, 0, W, 1 + l, W, 0, skip ? 0 : -1, skip ? np : 0);                                // layer l: [H_l | enc_pos] -> H_l+1
    }
    linear(3, 1, 1, Ln + 1, W, 0, -1, 0);                                                                   // density head: H_L
    linear(2, 0, W, Ln + 1, W, 0, -1, 0);                                                                   // feature layer: H_L -> F
    linear(1, 0, W / 2, Ln + 2, W, 0, 1, nd);                                                               // colour layer: [F | enc_dir] -> C_1
    linear(0, 1, 3, Ln + 3, W / 2, 0, -1, 0);                                                               // rgb head: C_1
    P.n_units = nu; P.n_lin = nl; P.chunk_floats = poff; P.total = off;
    for (int k = nu; k < NRC_NERF_MAX_UNITS; k++) P.u[k] = WUnit{0, 0, 0, 0, {0, 0}, {0, 0}, 0};
    for (int k = nl; k < NRC_NERF_MAX_LINEARS; k++) P.lin[k] = WLin{0, 0, {0, 0}, {0, 0}, 0, 0, off};
}

// grid (units, chunks).  Per 32-row tile the unit's operand and gradient fragments are copied (linear 16-byte loads, one tile ahead in registers) into an
// LDS tile TRANSPOSED -- [column][32 rows + 8] -- so that a lane reads the eight consecutive rows of its column, the K-major fragment of both MFMA
// operands, as one 16-byte LDS read.  Wave w owns gradient columns 32 w .. 32 w + 31 against every operand column; the bias is the lane's row sum.
__global__ void __launch_bounds__(256) k_nerf_wgrad(const uint4* __restrict__ ws, NerfWs S, WPlan P, int32_t chunk_tiles, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) _Float16 T[NRC_NERF_WG_COLS * NRC_NERF_WG_LD];
    const WUnit u = P.u[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hh = lane >> 5;
    const int64_t t0 = (int64_t)blockIdx.y * chunk_tiles, t1 = t0 + chunk_tiles < S.tiles32 ? t0 + chunk_tiles : S.tiles32;
    const int nx0 = u.x_nks[0] * 64, nx1 = u.x_nks[1] * 64, nfr = nx0 + nx1 + u.g_nks * 64;   // fragments (uint4) per tile: operand 0, operand 1, gradient
    const int xcols = 16 * (u.x_nks[0] + u.x_nks[1]), NT = xcols / 32, ocols = 16 * u.g_nks;
    const bool active = 32 * wave < ocols;
    for (int e = tid; e < NRC_NERF_WG_COLS * NRC_NERF_WG_LD / 8; e += 256) reinterpret_cast<uint4*>(T)[e] = make_uint4(0u, 0u, 0u, 0u);   // columns nobody writes stay 0

    // fragment e of a tile: where it comes from and the LDS column of its first element
    auto source = [&](int e, int64_t tile) -> const uint4* {
        if (e < nx0) return ws + S.stage_base(u.x_ks[0]) + tile * nx0 + e;
        if (e < nx0 + nx1) return ws + S.stage_base(u.x_ks[1]) + tile * nx1 + (e - nx0);
        return ws + S.stage_base(u.g_ks) + (tile * u.g_stage_nks + u.g_s0) * 64 + (e - nx0 - nx1);
    };
    uint4 pf[NRC_NERF_WG_PF];
    auto fetch = [&](int64_t tile) {
#pragma unroll
        for (int q = 0; q < NRC_NERF_WG_PF; q++) {
            const int e = tid + 256 * q;
            pf[q] = make_uint4(0u, 0u, 0u, 0u);
            if (e < nfr) pf[q] = *source(e, tile);
        }
    };
    f16v acc[NRC_NERF_WG_NT];
    zero_acc<NRC_NERF_WG_NT>(acc);
    float bsum = 0.f;
    if (t0 < t1) fetch(t0);
    for (int64_t tile = t0; tile < t1; tile++) {
        __syncthreads();   // the previous tile's fragments are read (and, first, the clear is done)
#pragma unroll
        for (int q = 0; q < NRC_NERF_WG_PF; q++) {
            const int e = tid + 256 * q;
            if (e < nfr) {
                // columns: operand 0, operand 1, gradient -- fragment e holds columns 16 (e / 64) + 8 hh' + j of that sequence for row e % 32
                const int col = 16 * (e >> 6) + 8 * ((e >> 5) & 1), row = e & 31;
                const h8 v = *reinterpret_cast<const h8*>(&pf[q]);
#pragma unroll
                for (int j = 0; j < 8; j++) T[(col + j) * NRC_NERF_WG_LD + row] = v[j];
            }
        }
        __syncthreads();
        if (tile + 1 < t1) fetch(tile + 1);
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const h8 a = *reinterpret_cast<const h8*>(&T[(xcols + 32 * wave + n) * NRC_NERF_WG_LD + 16 * ks + 8 * hh]);
#pragma unroll
                for (int j = 0; j < 8; j++) bsum += (float)a[j];
#pragma unroll
                for (int t = 0; t < NRC_NERF_WG_NT; t++)
                    if (t < NT) {
                        const h8 b = *reinterpret_cast<const h8*>(&T[(32 * t + n) * NRC_NERF_WG_LD + 16 * ks + 8 * hh]);
                        acc[t] = NRC_MFMA(a, b, acc[t]);
                    }
            }
        }
    }
    if (!active) return;
    float* out = partial + (size_t)blockIdx.y * P.chunk_floats + u.poff;
#pragma unroll
    for (int t = 0; t < NRC_NERF_WG_NT; t++)
        if (t < NT) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int o = 32 * wave + (reg & 3) + 8 * (reg >> 2) + 4 * hh;
                if (o < ocols) out[(size_t)o * xcols + 32 * t + n] = acc[t][reg];
            }
        }
    const float b = bsum + __shfl_xor(bsum, 32);
    if (hh == 0 && 32 * wave + n < ocols) out[(size_t)ocols * xcols + 32 * wave + n] = b;
}

// grad_params[idx] = (sum over the chunks, ascending) 2^-e; thread 0 also publishes the statistics
__global__ void __launch_bounds__(256) k_nerf_wreduce(const float* __restrict__ partial, WPlan P, int32_t n_chunks, const int32_t* __restrict__ hdr, int fixed,
                                                      int fixed_exp, float* __restrict__ grad, int32_t* __restrict__ stats) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const int e = scale_exponent(hdr, fixed, fixed_exp);
    if (idx == 0u) { stats[0] = e; stats[1] = hdr[1]; stats[2] = 0; stats[3] = 0; }
    if (idx >= P.total) return;
    int li = 0;
    while (li + 1 < P.n_lin && idx >= P.lin[li + 1].off) li++;
    const WLin q = P.lin[li];
    const uint32_t local = idx - q.off, nw = (uint32_t)(q.rows * q.ld);
    const int o = local < nw ? (int)(local / (uint32_t)q.ld) : (int)(local - nw), oc = frag_col(o, q.gnat);
    const WUnit u = P.u[q.unit0 + (oc >> 7)];
    const int xcols = 16 * (u.x_nks[0] + u.x_nks[1]), ocols = 16 * u.g_nks, ol = oc & 127;
    uint32_t at;
    if (local < nw) {
        const int i = (int)(local % (uint32_t)q.ld);
        const int col = i < q.xw[0] ? frag_col(i, q.xnat[0]) : 16 * u.x_nks[0] + frag_col(i - q.xw[0], q.xnat[1]);
        at = u.poff + (uint32_t)(ol * xcols + col);
    } else {
        at = u.poff + (uint32_t)(ocols * xcols + ol);
    }
    float sum = 0.f;
    for (int ch = 0; ch < n_chunks; ch++) sum = __fadd_rn(sum, partial[(size_t)ch * P.chunk_floats + at]);
    grad[idx] = __fmul_rn(sum, pow2f(-e));
}

// one stage of the workspace as (M, width) row-major fp16 (tests)
__global__ void __launch_bounds__(256) k_nerf_read_stage(const uint4* __restrict__ ws, int64_t base, int32_t nks, int32_t width, int32_t natural, int64_t M,
                                                         _Float16* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * width) return;
    const int64_t row = idx / width;
    const int col = frag_col((int)(idx % width), natural), lane = 32 * ((col >> 3) & 1) + (int)(row & 31);
    out[idx] = reinterpret_cast<const _Float16*>(ws + base + ((row >> 5) * nks + (col >> 4)) * 64 + lane)[col & 7];
}

int read_stage(const void* workspace, const NerfCfg& c, int64_t M, int ks, int nks, int width, int natural, void* out, hipStream_t s) {
    if (M == 0) return NRC_OK;
    if (!workspace || !out || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return NRC_ERR_INVALID;
    const NerfWs S = make_ws(c, M);
    const int64_t blocks = nrc_cdiv(M * width, 256);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    hipLaunchKernelGGL(k_nerf_read_stage, dim3((unsigned)blocks), dim3(256), 0, s, (const uint4*)workspace, S.stage_base(ks), nks, width, natural, M, (_Float16*)out);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // namespace

extern "C" {

int nrc_nerf_wgrad_chunk_rows(void) { return NRC_NERF_WGRAD_CHUNK_ROWS; }

int64_t nrc_nerf_train_workspace_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                                       int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, int64_t M) {
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (M < 0) return NRC_ERR_INVALID;
    const NerfWs S = make_ws(c, M);
    WPlan P;
    make_plan(c, S, P);
    return S.partial_base() * 16 + nrc_cdiv(S.tiles32 * 32, NRC_NERF_WGRAD_CHUNK_ROWS) * (int64_t)P.chunk_floats * 4;
}

int64_t nrc_nerf_grad_params_floats(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                                    int32_t append_input, int32_t skip_mask) {
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    WPlan P;
    make_plan(c, make_ws(c, 0), P);
    return (int64_t)P.total;
}

int64_t nrc_nerf_packed_transposed_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                                         int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask) {
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    NerfLayout L;
    make_layout_t(c, L);
    return (int64_t)L.w_total * 16;
}

int nrc_nerf_pack_weights_transposed(const float* const* params, int32_t n_params, int32_t width, int32_t n_layers, int32_t n_color_layers,
                                     int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, void* blob,
                                     nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (!params || !blob || (reinterpret_cast<uintptr_t>(blob) & 15u)) return NRC_ERR_INVALID;
    if (n_params != 2 * (n_layers + 4)) return NRC_ERR_INVALID;
    NerfLayout L;
    make_layout_t(c, L);
    NerfParams P;
    for (int k = 0; k < 2 * NRC_NERF_MAX_LINEARS; k++) {
        P.p[k] = k < n_params ? params[k] : nullptr;
        if (k < n_params && !P.p[k]) return NRC_ERR_INVALID;
    }
    NRC_STAGE((hipStream_t)stream, nullptr);
    hipLaunchKernelGGL(k_nerf_pack_t, dim3((L.w_total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, P, L, (uint4*)blob);
    NRC_LAUNCH_CHECK();
    NRC_STAGE((hipStream_t)stream, "k_nerf_pack_t");
    return NRC_OK;
}

int nrc_nerf_block_backward(const float* d_sigma, const float* d_rgb, const float* sigma, const float* rgb, int64_t M, const void* blob_transposed,
                            int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                            int32_t append_input, int32_t skip_mask, void* workspace, float grad_scale, float* grad_params, int32_t* stats,
                            nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    int fixed = 0, fixed_exp = 0;
    if (grad_scale != 0.f) {   // a positive power of two inside the range the kernels can invert
        if (!(grad_scale > 0.f) || frexpf(grad_scale, &fixed_exp) != 0.5f) return NRC_ERR_INVALID;
        fixed = 1;
        fixed_exp -= 1;
        if (fixed_exp < -126 || fixed_exp > 126) return NRC_ERR_INVALID;
    }
    if (M < 0) return NRC_ERR_INVALID;
    if (M == 0) return NRC_OK;
    if (!d_sigma || !d_rgb || !sigma || !rgb || !blob_transposed || !workspace || !grad_params || !stats ||
        (reinterpret_cast<uintptr_t>(blob_transposed) & 15u) || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return NRC_ERR_INVALID;
    const int64_t blocks = nrc_cdiv(M, NRC_NERF_TILE_ROWS);
    if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    const NerfWs S = make_ws(c, M);
    NerfLayout L;
    make_layout_t(c, L);
    WPlan P;
    make_plan(c, S, P);
    const int chunk_tiles = NRC_NERF_WGRAD_CHUNK_ROWS / 32;
    const int64_t n_chunks = nrc_cdiv(S.tiles32, chunk_tiles);
    if (n_chunks > 65535) return NRC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    uint4* ws = (uint4*)workspace;
    int32_t* hdr = (int32_t*)workspace;
    float* partial = reinterpret_cast<float*>(ws + S.partial_base());
    NRC_STAGE(s, nullptr);
    if (nrc_zero_async(hdr, NRC_NERF_WS_HEADER * 16, s) != hipSuccess) return NRC_ERR_LAUNCH;
    if (!fixed) hipLaunchKernelGGL(k_nerf_head_max, dim3((unsigned)nrc_cdiv(M, 256)), dim3(256), 0, s, d_sigma, d_rgb, sigma, rgb, M, hdr);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_head_max");
    if (width == 256) hipLaunchKernelGGL((k_nerf_dgrad<256>), dim3((unsigned)blocks), dim3(256), 0, s, d_sigma, d_rgb, sigma, rgb, M, (const uint4*)blob_transposed, c, L, ws, fixed, fixed_exp);
    else hipLaunchKernelGGL((k_nerf_dgrad<128>), dim3((unsigned)blocks), dim3(256), 0, s, d_sigma, d_rgb, sigma, rgb, M, (const uint4*)blob_transposed, c, L, ws, fixed, fixed_exp);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_dgrad");
    hipLaunchKernelGGL(k_nerf_wgrad, dim3((unsigned)P.n_units, (unsigned)n_chunks), dim3(256), 0, s, (const uint4*)ws, S, P, chunk_tiles, partial);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_wgrad");
    hipLaunchKernelGGL(k_nerf_wreduce, dim3((P.total + 255u) / 256u), dim3(256), 0, s, (const float*)partial, P, (int32_t)n_chunks, (const int32_t*)hdr, fixed,
                       fixed_exp, grad_params, stats);
    NRC_LAUNCH_CHECK();
    NRC_STAGE(s, "k_nerf_wreduce");
    return NRC_OK;
}

int nrc_nerf_saved_stage(const void* workspace, int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                         int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, int64_t M, int32_t stage, void* out, nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (M < 0 || stage < 0 || stage > n_layers + 3) return NRC_ERR_INVALID;
    const NerfWs S = make_ws(c, M);
    const int wd = stage == 0 ? enc_width(c.n_freq_pos, c.append_input) : (stage == 1 ? enc_width(c.n_freq_dir, c.append_input) : (stage == n_layers + 3 ? width / 2 : width));
    return read_stage(workspace, c, M, S.saved_ks(stage), S.saved_nks(stage), wd, stage < 2, out, (hipStream_t)stream);
}

int nrc_nerf_grad_stage(const void* workspace, int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                        int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, int64_t M, int32_t stage, void* out, nrc_stream_t stream) {
    NRC_ENTER();
    const NerfCfg c{width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask};
    if (!train_cfg_supported(c)) return NRC_ERR_UNSUPPORTED;
    if (M < 0 || stage < 0 || stage > n_layers + 3) return NRC_ERR_INVALID;
    const NerfWs S = make_ws(c, M);
    const int wd = stage == 0 ? 3 : (stage == 3 ? 1 : (stage == 1 ? width / 2 : width));
    return read_stage(workspace, c, M, S.grad_ks(stage), S.grad_nks(stage), wd, stage == 0 || stage == 3, out, (hipStream_t)stream);
}

}  // extern "C"
