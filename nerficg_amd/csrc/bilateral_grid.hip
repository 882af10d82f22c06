// bilateral_grid.hip -- per-image colour correction by a bilateral grid of 3 x 4 affine transforms (Wang et al., Bilateral Guided Radiance Field Processing,
// SIGGRAPH 2024; gsplat: use_bilateral_grid): slice + apply, its two gradients and the total-variation term (include/nerficg_hip.h group 28, which states
// the definition).  Grids (N, 12, L, Gh, Gw) f32, channel c = 4 r + k is entry (r, k).  The written f32 sequence below is the one tests/bilateral_grid_ref.py
// counts rounding by rounding (the translation unit is built with -ffp-contract=off, see build.py):
//
//   u = (x + 0.5f) / W, v = (y + 0.5f) / H, g = (0.299f p0 + 0.587f p1) + 0.114f p2
//   per axis: c = clamp(t, 0, 1) (n - 1); i = min(floor(c), n - 2); f = c - i; w0 = 1 - f, w1 = f          (n == 1: i = 0, f = 0, the second vertex IS the first)
//   A_c = sum over (dy, dx) in (0,0) (0,1) (1,0) (1,1), z0 then z1, of (wz (wy wx)) G       D_c = sum over (dy, dx) of (wy wx) (G[z1] - G[z0])
//   out_r = ((A(r,0) p0 + A(r,1) p1) + A(r,2) p2) + A(r,3)
//   d_p_k = ((d0 A(0,k) + d1 A(1,k)) + d2 A(2,k)) + coef_k (S (L - 1)),  S = (d0 s0 + d1 s1) + d2 s2,  s_r = ((D(r,0) p0 + D(r,1) p1) + D(r,2) p2) + D(r,3)
//            (the guidance part only where 0 <= g <= 1: at g == 1 the clamp leaves i = L - 2, f = 1, the last cell's slope)
//   d_G[vertex, 4 r + k] = sum over pixels of (wz (wy wx)) (d_r q_k), q = (p0, p1, p2, 1)
//
// TILES: a workgroup of 256 lanes takes 32 x 8 pixels, one lane per pixel.  The vertex window of a tile is [i(first pixel), i(last pixel) + 1] along x and y
// and all L levels; i() is monotone in the pixel index (every f32 operation in it is), so every lane's eight corners lie inside.  The host evaluates the same
// function over the tile columns and rows and hands the launch the largest window (wnx, wny).  Where wnx wny L 12 floats fit BG_WCAP the kernels stage the
// window in LDS, the 12 coefficients of a vertex contiguous (k_bilagrid_slice<true>, k_bilagrid_slice_bw<true>); where they do not -- small images under
// large grids -- every tile of that launch loads its corners from memory (<false>) and the grid gradient is gathered per vertex (k_bilagrid_gather).
//
// GRID GRADIENT, the same bits on every call, no atomics: in k_bilagrid_slice_bw<true> a wave visits every vertex of the window once (skipping, by ballot,
// those no lane touches), sums the 12 products over its 64 lanes with a fixed butterfly and stores them into its own copy of the window in LDS; the four
// copies are added as (w0 + w1) + (w2 + w3) and the workgroup writes ONE partial window into the workspace.  k_bilagrid_reduce then sums, per grid entry, the
// partials of the tiles whose window holds it, in tile order, with a double accumulator, and writes slice n of d_grids and zeros into every other slice.
// k_bilagrid_gather (the direct path) sums, per vertex, over the pixels that touch it in pixel order, also in double.
//
// TV: k_bilagrid_tv squares the f32 forward differences and sums them in double (per axis; a fixed butterfly, one partial triple per workgroup),
// k_bilagrid_tv_final adds the partials in order and scales; k_bilagrid_tv_bw is the stencil.
#include <math.h>

#include "common.h"

namespace {

constexpr int BG_TX = 32, BG_TY = 8, BG_N = 256;   // pixel tile and workgroup
constexpr int BG_WCAP = 1536;                      // floats of one staged window: 16 x-y vertices x 8 levels x 12 (3 x 3 at 1297 x 840 under 16 x 16 x 8)
constexpr int BG_TV_BLOCKS = 1024;                 // workgroups (and partial triples) of k_bilagrid_tv at the most
constexpr float BG_CR = 0.299f, BG_CG = 0.587f, BG_CB = 0.114f;

// cell index and fraction of coordinate t along an axis of n vertices.  A NaN coordinate takes cell 0.
__host__ __device__ __forceinline__ void bg_axis(float t, int n, int& i, float& f) {
    if (n == 1) { i = 0; f = 0.f; return; }
    const float tc = !(t > 0.f) ? 0.f : (t > 1.f ? 1.f : t);
    const float c = tc * (float)(n - 1);
    int fi = (int)floorf(c);
    fi = fi < n - 2 ? fi : n - 2;
    i = fi < 0 ? 0 : fi;
    f = c - (float)i;
}
__host__ __device__ __forceinline__ int bg_cell_of_pixel(int p, int extent, int n) {
    int i; float f;
    bg_axis(((float)p + 0.5f) / (float)extent, n, i, f);
    return i;
}
// vertex range [lo, hi] of the pixels [p0, p0 + len) (clipped to the image) along an axis
__host__ __device__ __forceinline__ void bg_window(int p0, int len, int extent, int n, int& lo, int& hi) {
    const int p1 = p0 + len - 1 < extent - 1 ? p0 + len - 1 : extent - 1;
    lo = bg_cell_of_pixel(p0, extent, n);
    hi = bg_cell_of_pixel(p1, extent, n) + (n > 1 ? 1 : 0);
}

struct BgShape { int L, Gh, Gw, H, W; };

__device__ __forceinline__ int bg_index(int idx_host, const int32_t* __restrict__ idx_dev, int N) {
    int n = idx_dev ? idx_dev[0] : idx_host;
    n = n < 0 ? 0 : (n >= N ? N - 1 : n);   // a device index outside [0, N) is clamped: memory safety only (the host integer is validated)
    return n;
}

// what one pixel knows about its place in the grid
struct BgPix {
    int ix, iy, iz;
    float wx[2], wy[2], wz[2];
    float g;
};
__device__ __forceinline__ BgPix bg_place(int x, int y, float p0, float p1, float p2, const BgShape& s) {
    BgPix q;
    float f;
    bg_axis(((float)x + 0.5f) / (float)s.W, s.Gw, q.ix, f); q.wx[0] = 1.f - f; q.wx[1] = f;
    bg_axis(((float)y + 0.5f) / (float)s.H, s.Gh, q.iy, f); q.wy[0] = 1.f - f; q.wy[1] = f;
    q.g = (BG_CR * p0 + BG_CG * p1) + BG_CB * p2;
    bg_axis(q.g, s.L, q.iz, f); q.wz[0] = 1.f - f; q.wz[1] = f;
    return q;
}

// A (and D = dA/dc_z) of one pixel.  LDSW: the coefficients come from the staged window `win` (origin (wy0, wx0), pitch wnx vertices, 12 floats per vertex),
// else from the grid `G` (12, L, Gh, Gw) itself.
template <bool LDSW, bool WITH_D>
__device__ __forceinline__ void bg_sample(const BgPix& q, const BgShape& s, const float* __restrict__ G, const float* win, int wx0, int wy0, int wnx, int wny,
                                          float (&A)[12], float (&D)[12]) {
    const int sx = s.Gw > 1, sy = s.Gh > 1, sz = s.L > 1;
    const size_t cstride = (size_t)s.L * s.Gh * s.Gw;
#pragma unroll
    for (int c = 0; c < 12; c++) { A[c] = 0.f; D[c] = 0.f; }
    // one x-y corner per turn, not unrolled: unrolled, the 24 window loads of a pixel are hoisted together (178 VGPRs in the backward kernel, two waves per SIMD)
#pragma unroll 1
    for (int corner = 0; corner < 4; corner++) {
        {
            const int dy = corner >> 1, dx = corner & 1;
            const float wyx = (dy ? q.wy[1] : q.wy[0]) * (dx ? q.wx[1] : q.wx[0]);
            const float w0 = q.wz[0] * wyx, w1 = q.wz[1] * wyx;
            const int vy = q.iy + dy * sy, vx = q.ix + dx * sx;
            if (LDSW) {
                int ly = vy - wy0, lx = vx - wx0;
                ly = ly < 0 ? 0 : (ly > wny - 1 ? wny - 1 : ly);   // inside by construction (see TILES); the clamps keep a wrong window a wrong number
                lx = lx < 0 ? 0 : (lx > wnx - 1 ? wnx - 1 : lx);
                const float4* v0 = reinterpret_cast<const float4*>(win + (size_t)((ly * wnx + lx) * s.L + q.iz) * 12);
                const float4* v1 = v0 + 3 * sz;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float4 a = v0[j], b = v1[j];
                    const float g0[4] = {a.x, a.y, a.z, a.w}, g1[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        A[4 * j + k] += w0 * g0[k];
                        A[4 * j + k] += w1 * g1[k];
                        if (WITH_D) D[4 * j + k] += wyx * (g1[k] - g0[k]);
                    }
                }
            } else {
                const size_t o0 = ((size_t)q.iz * s.Gh + vy) * s.Gw + vx, o1 = o0 + (size_t)sz * s.Gh * s.Gw;
#pragma unroll
                for (int c = 0; c < 12; c++) {
                    const float g0 = G[c * cstride + o0], g1 = G[c * cstride + o1];
                    A[c] += w0 * g0;
                    A[c] += w1 * g1;
                    if (WITH_D) D[c] += wyx * (g1 - g0);
                }
            }
        }
    }
}

// the tile's window of grid G into LDS: win[((ly * wnx + lx) * L + z) * 12 + c]; entries of the (wny, wnx) rectangle beyond the grid are zero
__device__ __forceinline__ void bg_stage(float* win, const float* __restrict__ G, const BgShape& s, int wx0, int wy0, int wnx, int wny) {
    const int n = wnx * wny * s.L * 12;
    for (int k = threadIdx.x; k < n; k += BG_N) {
        int r = k;
        const int lx = r % wnx; r /= wnx;
        const int ly = r % wny; r /= wny;
        const int z = r % s.L;
        const int c = r / s.L;
        const int vy = wy0 + ly, vx = wx0 + lx;
        float v = 0.f;
        if (vy < s.Gh && vx < s.Gw) v = G[(((size_t)c * s.L + z) * s.Gh + vy) * s.Gw + vx];
        win[((ly * wnx + lx) * s.L + z) * 12 + c] = v;
    }
}

template <bool LDSW>
__global__ void __launch_bounds__(BG_N) k_bilagrid_slice(const float* __restrict__ grids, int N, BgShape s, const float* __restrict__ rgb, int64_t ps, int64_t cs,
                                                         int idx_host, const int32_t* __restrict__ idx_dev, int wnx, int wny, float* __restrict__ out,
                                                         float* __restrict__ affine) {
    __shared__ __attribute__((aligned(16))) float win[LDSW ? BG_WCAP : 4];
    const int n = bg_index(idx_host, idx_dev, N);
    const float* G = grids + (size_t)n * 12 * s.L * s.Gh * s.Gw;
    const int x0 = blockIdx.x * BG_TX, y0 = blockIdx.y * BG_TY;
    int wx0 = 0, wy0 = 0, hi;
    if (LDSW) {
        bg_window(x0, BG_TX, s.W, s.Gw, wx0, hi);
        bg_window(y0, BG_TY, s.H, s.Gh, wy0, hi);
        bg_stage(win, G, s, wx0, wy0, wnx, wny);
        __syncthreads();
    }
    const int x = x0 + (threadIdx.x & 31), y = y0 + (threadIdx.x >> 5);
    if (x >= s.W || y >= s.H) return;
    const size_t pix = (size_t)y * s.W + x;
    const size_t o = pix * (size_t)ps;
    const float p0 = rgb[o], p1 = rgb[o + (size_t)cs], p2 = rgb[o + 2 * (size_t)cs];
    const BgPix q = bg_place(x, y, p0, p1, p2, s);
    float A[12], D[12];
    bg_sample<LDSW, false>(q, s, G, win, wx0, wy0, wnx, wny, A, D);
#pragma unroll
    for (int r = 0; r < 3; r++) out[o + r * (size_t)cs] = ((A[4 * r] * p0 + A[4 * r + 1] * p1) + A[4 * r + 2] * p2) + A[4 * r + 3];
    if (affine) {
        float4* a = reinterpret_cast<float4*>(affine + pix * 12);
#pragma unroll
        for (int j = 0; j < 3; j++) a[j] = make_float4(A[4 * j], A[4 * j + 1], A[4 * j + 2], A[4 * j + 3]);
    }
}

// weight of grid vertex v for a pixel in cell i with weights (w[0], w[1]) along an axis of step st (0: one vertex only)
__device__ __forceinline__ float bg_sel(int v, int i, int st, const float (&w)[2]) {
    return (v == i ? w[0] : 0.f) + ((st && v == i + 1) ? w[1] : 0.f);   // one of the two is zero: exact
}

// d_rgb, and (LDSW, partial != NULL) the tile's partial window of the grid gradient: partial[tile][(ly * wnx + lx) * L + z) * 12 + c]
template <bool LDSW>
__global__ void __launch_bounds__(BG_N) k_bilagrid_slice_bw(const float* __restrict__ grids, int N, BgShape s, const float* __restrict__ rgb,
                                                            const float* __restrict__ d_out, int64_t ps, int64_t cs, int idx_host,
                                                            const int32_t* __restrict__ idx_dev, int wnx, int wny, float* __restrict__ d_rgb,
                                                            float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float win[LDSW ? BG_WCAP : 4];
    __shared__ float acc[LDSW ? 4 * BG_WCAP : 4];
    const int n = bg_index(idx_host, idx_dev, N);
    const float* G = grids + (size_t)n * 12 * s.L * s.Gh * s.Gw;
    const int x0 = blockIdx.x * BG_TX, y0 = blockIdx.y * BG_TY;
    int wx0 = 0, wy0 = 0, wx1 = 0, wy1 = 0;
    const int wfloats = wnx * wny * s.L * 12;
    if (LDSW) {
        bg_window(x0, BG_TX, s.W, s.Gw, wx0, wx1);
        bg_window(y0, BG_TY, s.H, s.Gh, wy0, wy1);
        bg_stage(win, G, s, wx0, wy0, wnx, wny);
        if (partial)
            for (int k = threadIdx.x; k < 4 * BG_WCAP; k += BG_N) acc[k] = 0.f;
        __syncthreads();
    }
    const int x = x0 + (threadIdx.x & 31), y = y0 + (threadIdx.x >> 5);
    const bool valid = x < s.W && y < s.H;
    const size_t o = valid ? ((size_t)y * s.W + x) * (size_t)ps : 0;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, d[3] = {0.f, 0.f, 0.f};
    if (valid) {
        p0 = rgb[o]; p1 = rgb[o + (size_t)cs]; p2 = rgb[o + 2 * (size_t)cs];
        d[0] = d_out[o]; d[1] = d_out[o + (size_t)cs]; d[2] = d_out[o + 2 * (size_t)cs];
    }
    const BgPix q = bg_place(valid ? x : x0, valid ? y : y0, p0, p1, p2, s);
    if (valid && d_rgb) {
        float A[12], D[12];
        bg_sample<LDSW, true>(q, s, G, win, wx0, wy0, wnx, wny, A, D);
        float sl[3];
#pragma unroll
        for (int r = 0; r < 3; r++) sl[r] = ((D[4 * r] * p0 + D[4 * r + 1] * p1) + D[4 * r + 2] * p2) + D[4 * r + 3];
        const float S = (d[0] * sl[0] + d[1] * sl[1]) + d[2] * sl[2];
        const float gz = (q.g >= 0.f && q.g <= 1.f) ? S * (float)(s.L - 1) : 0.f;
        const float coef[3] = {BG_CR, BG_CG, BG_CB};
#pragma unroll
        for (int k = 0; k < 3; k++) d_rgb[o + k * (size_t)cs] = ((d[0] * A[k] + d[1] * A[4 + k]) + d[2] * A[8 + k]) + coef[k] * gz;
    }
    if (!LDSW || !partial) return;
    // the grid gradient: every vertex of the tile's window once per wave
    float m[12];
#pragma unroll
    for (int r = 0; r < 3; r++) { m[4 * r] = d[r] * p0; m[4 * r + 1] = d[r] * p1; m[4 * r + 2] = d[r] * p2; m[4 * r + 3] = d[r]; }
    const int sx = s.Gw > 1, sy = s.Gh > 1, sz = s.L > 1;
    const int lane = threadIdx.x & 63;
    float* mine = acc + (threadIdx.x >> 6) * BG_WCAP;
    int ny = wy1 - wy0 + 1, nx = wx1 - wx0 + 1;
    ny = ny < wny ? ny : wny; nx = nx < wnx ? nx : wnx;
    for (int ly = 0; ly < ny; ly++) {
        const float wys = valid ? bg_sel(wy0 + ly, q.iy, sy, q.wy) : 0.f;
        for (int lx = 0; lx < nx; lx++) {
            const float wyx = wys * bg_sel(wx0 + lx, q.ix, sx, q.wx);
            if (__ballot(wyx != 0.f) == 0) continue;
            for (int z = 0; z < s.L; z++) {
                const float w = bg_sel(z, q.iz, sz, q.wz) * wyx;
                if (__ballot(w != 0.f) == 0) continue;
                float* dst = mine + ((ly * wnx + lx) * s.L + z) * 12;
#pragma unroll
                for (int c = 0; c < 12; c++) {
                    const float v = nrc_group_sum<64>(w * m[c]);
                    if (lane == 0) dst[c] = v;
                }
            }
        }
    }
    __syncthreads();
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    float* dstp = partial + tile * (size_t)wfloats;
    for (int k = threadIdx.x; k < wfloats; k += BG_N) dstp[k] = (acc[k] + acc[BG_WCAP + k]) + (acc[2 * BG_WCAP + k] + acc[3 * BG_WCAP + k]);
}

// d_grids (N, 12, L, Gh, Gw): slice n from the partial windows, zero elsewhere.  One thread per element; inside slice n the threads are dealt in the
// partials' order (y, x, z, c), so that a wave reads runs of a tile's window.
__global__ void __launch_bounds__(BG_N) k_bilagrid_reduce(const float* __restrict__ partial, int N, BgShape s, int idx_host, const int32_t* __restrict__ idx_dev,
                                                          int wnx, int wny, int ntx, int nty, float* __restrict__ d_grids) {
    const size_t E = (size_t)12 * s.L * s.Gh * s.Gw;
    const size_t gid = (size_t)blockIdx.x * BG_N + threadIdx.x;
    if (gid >= (size_t)N * E) return;
    const int n = bg_index(idx_host, idx_dev, N);
    const size_t slice = gid / E;
    if ((int)slice != n) { d_grids[gid] = 0.f; return; }
    size_t r = gid - slice * E;
    const int c = (int)(r % 12); r /= 12;
    const int z = (int)(r % s.L); r /= s.L;
    const int vx = (int)(r % s.Gw);
    const int vy = (int)(r / s.Gw);
    // the tile columns / rows whose window holds the vertex: a run, the windows' ends are monotone
    int txa = ntx, txb = -1, tya = nty, tyb = -1;
    for (int t = 0; t < ntx; t++) {
        int lo, hi;
        bg_window(t * BG_TX, BG_TX, s.W, s.Gw, lo, hi);
        if (lo <= vx && vx <= hi) { txa = t < txa ? t : txa; txb = t; }
    }
    for (int t = 0; t < nty; t++) {
        int lo, hi;
        bg_window(t * BG_TY, BG_TY, s.H, s.Gh, lo, hi);
        if (lo <= vy && vy <= hi) { tya = t < tya ? t : tya; tyb = t; }
    }
    const size_t wfloats = (size_t)wnx * wny * s.L * 12;
    double sum = 0.0;
    for (int ty = tya; ty <= tyb; ty++) {
        const int ly = vy - bg_cell_of_pixel(ty * BG_TY, s.H, s.Gh);
        if (ly < 0 || ly >= wny) continue;
        for (int tx = txa; tx <= txb; tx++) {
            const int lx = vx - bg_cell_of_pixel(tx * BG_TX, s.W, s.Gw);
            if (lx < 0 || lx >= wnx) continue;
            sum += (double)partial[((size_t)ty * ntx + tx) * wfloats + (size_t)((ly * wnx + lx) * s.L + z) * 12 + c];
        }
    }
    d_grids[slice * E + (((size_t)c * s.L + z) * s.Gh + vy) * s.Gw + vx] = (float)sum;
}

// first pixel p in [0, extent) whose cell index is >= want (extent when there is none)
__device__ __forceinline__ int bg_first_pixel(int want, int extent, int n) {
    int lo = 0, hi = extent;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bg_cell_of_pixel(mid, extent, n) >= want) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the direct path's grid gradient: one thread per (slice, z, y, x) vertex, 12 double sums over the pixels that touch it, in pixel order
__global__ void __launch_bounds__(BG_N) k_bilagrid_gather(int N, BgShape s, const float* __restrict__ rgb, const float* __restrict__ d_out, int64_t ps, int64_t cs,
                                                          int idx_host, const int32_t* __restrict__ idx_dev, float* __restrict__ d_grids) {
    const size_t V = (size_t)s.L * s.Gh * s.Gw;
    const size_t gid = (size_t)blockIdx.x * BG_N + threadIdx.x;
    if (gid >= (size_t)N * V) return;
    const int n = bg_index(idx_host, idx_dev, N);
    const size_t slice = gid / V;
    size_t r = gid - slice * V;
    float* dst = d_grids + slice * 12 * V + r;
    double sum[12];
#pragma unroll
    for (int c = 0; c < 12; c++) sum[c] = 0.0;
    if ((int)slice == n) {
        const int vx = (int)(r % s.Gw); r /= s.Gw;
        const int vy = (int)(r % s.Gh);
        const int vz = (int)(r / s.Gh);
        const int sx = s.Gw > 1, sy = s.Gh > 1, sz = s.L > 1;
        const int xa = bg_first_pixel(vx - 1, s.W, s.Gw), xb = bg_first_pixel(vx + 1, s.W, s.Gw);
        const int ya = bg_first_pixel(vy - 1, s.H, s.Gh), yb = bg_first_pixel(vy + 1, s.H, s.Gh);
        for (int y = ya; y < yb; y++) {
            for (int x = xa; x < xb; x++) {
                const size_t o = ((size_t)y * s.W + x) * (size_t)ps;
                const float p0 = rgb[o], p1 = rgb[o + (size_t)cs], p2 = rgb[o + 2 * (size_t)cs];
                const BgPix q = bg_place(x, y, p0, p1, p2, s);
                const float wyx = bg_sel(vy, q.iy, sy, q.wy) * bg_sel(vx, q.ix, sx, q.wx);
                const float w = bg_sel(vz, q.iz, sz, q.wz) * wyx;
                if (w == 0.f) continue;
                const float d[3] = {d_out[o], d_out[o + (size_t)cs], d_out[o + 2 * (size_t)cs]};
#pragma unroll
                for (int rr = 0; rr < 3; rr++) {
                    sum[4 * rr] += (double)(w * (d[rr] * p0));
                    sum[4 * rr + 1] += (double)(w * (d[rr] * p1));
                    sum[4 * rr + 2] += (double)(w * (d[rr] * p2));
                    sum[4 * rr + 3] += (double)(w * d[rr]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 12; c++) dst[c * V] = (float)sum[c];
}

// ---------------------------------------------------------------------------------------------------- total variation
// sums of squared forward differences along z, y, x over a run of elements, in double; partial3[3 * block + axis]
__global__ void __launch_bounds__(BG_N) k_bilagrid_tv(const float* __restrict__ grids, size_t total, int L, int Gh, int Gw, double* __restrict__ partial3) {
    __shared__ double red[3][BG_N / 64];
    double az = 0.0, ay = 0.0, ax = 0.0;
    const size_t sy = (size_t)Gw, szz = (size_t)Gh * Gw;
    for (size_t e = (size_t)blockIdx.x * BG_N + threadIdx.x; e < total; e += (size_t)gridDim.x * BG_N) {
        const int x = (int)(e % Gw);
        const int y = (int)((e / Gw) % Gh);
        const int z = (int)((e / szz) % L);
        const float v = grids[e];
        if (z + 1 < L) { const float dd = grids[e + szz] - v; az += (double)dd * (double)dd; }
        if (y + 1 < Gh) { const float dd = grids[e + sy] - v; ay += (double)dd * (double)dd; }
        if (x + 1 < Gw) { const float dd = grids[e + 1] - v; ax += (double)dd * (double)dd; }
    }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) { az += __shfl_xor(az, dl, 64); ay += __shfl_xor(ay, dl, 64); ax += __shfl_xor(ax, dl, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = az; red[1][threadIdx.x >> 6] = ay; red[2][threadIdx.x >> 6] = ax; }
    __syncthreads();
    if (threadIdx.x < 3) partial3[3 * (size_t)blockIdx.x + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// tv = (sum_z inv_z + sum_y inv_y + sum_x inv_x), inv_a = 1 / (N count_a) (0 for an axis of extent 1); one wave, the partials in order
__global__ void __launch_bounds__(64) k_bilagrid_tv_final(const double* __restrict__ partial3, int n_blocks, double inv_z, double inv_y, double inv_x, float* __restrict__ tv) {
    double a[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < n_blocks; k += 64) { a[0] += partial3[3 * k]; a[1] += partial3[3 * k + 1]; a[2] += partial3[3 * k + 2]; }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) { a[0] += __shfl_xor(a[0], dl, 64); a[1] += __shfl_xor(a[1], dl, 64); a[2] += __shfl_xor(a[2], dl, 64); }
    if (threadIdx.x == 0) tv[0] = (float)((a[0] * inv_z + a[1] * inv_y) + a[2] * inv_x);
}

// d_G = (g kz) Sz + (g ky) Sy + (g kx) Sx, S_a = (G[i] - G[i-1]) - (G[i+1] - G[i]) with the missing neighbour's difference left out, k_a = 2 / (N count_a)
__global__ void __launch_bounds__(BG_N) k_bilagrid_tv_bw(const float* __restrict__ grids, size_t total, int L, int Gh, int Gw, float kz, float ky, float kx,
                                                         const float* __restrict__ upstream, float* __restrict__ d_grids) {
    const size_t e = (size_t)blockIdx.x * BG_N + threadIdx.x;
    if (e >= total) return;
    const float g = upstream ? upstream[0] : 1.f;
    const size_t sy = (size_t)Gw, szz = (size_t)Gh * Gw;
    const int x = (int)(e % Gw);
    const int y = (int)((e / Gw) % Gh);
    const int z = (int)((e / szz) % L);
    const float v = grids[e];
    float s3[3];
    const int pos[3] = {z, y, x}, ext[3] = {L, Gh, Gw};
    const size_t st[3] = {szz, sy, 1};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float sa = 0.f;
        if (pos[a] >= 1) sa = v - grids[e - st[a]];
        if (pos[a] + 1 < ext[a]) sa = sa - (grids[e + st[a]] - v);
        s3[a] = sa;
    }
    d_grids[e] = ((g * kz) * s3[0] + (g * ky) * s3[1]) + (g * kx) * s3[2];
}

bool bg_grid_ok(int64_t N, int32_t L, int32_t Gh, int32_t Gw) {
    return N >= 1 && L >= 1 && Gh >= 1 && Gw >= 1 && L <= 4096 && Gh <= 4096 && Gw <= 4096 && N <= 0x7fffffff && N * 12 * (int64_t)L * Gh * Gw <= ((int64_t)1 << 38);
}
bool bg_image_ok(int32_t H, int32_t W) { return H >= 0 && W >= 0 && (int64_t)H * W <= ((int64_t)1 << 30); }

// the largest vertex window of a 32 x 8 tile, from the function the kernels evaluate
void bg_max_window(const BgShape& s, int& wnx, int& wny) {
    wnx = wny = 1;
    for (int x0 = 0; x0 < s.W; x0 += BG_TX) { int lo, hi; bg_window(x0, BG_TX, s.W, s.Gw, lo, hi); wnx = hi - lo + 1 > wnx ? hi - lo + 1 : wnx; }
    for (int y0 = 0; y0 < s.H; y0 += BG_TY) { int lo, hi; bg_window(y0, BG_TY, s.H, s.Gh, lo, hi); wny = hi - lo + 1 > wny ? hi - lo + 1 : wny; }
}
bool bg_window_fits(const BgShape& s, int wnx, int wny) { return (int64_t)wnx * wny * s.L * 12 <= BG_WCAP; }

int64_t bg_tv_blocks(int64_t total) { const int64_t b = nrc_cdiv(total, BG_N); return b < BG_TV_BLOCKS ? b : BG_TV_BLOCKS; }

}  // namespace

extern "C" {

int64_t nrc_bilagrid_ws_floats(int64_t N, int32_t L, int32_t Gh, int32_t Gw, int32_t H, int32_t W) {
    if (!bg_grid_ok(N, L, Gh, Gw) || !bg_image_ok(H, W)) return NRC_ERR_INVALID;
    const BgShape s{L, Gh, Gw, H, W};
    int64_t need = 2 * 3 * (int64_t)BG_TV_BLOCKS;   // k_bilagrid_tv's partial triples, doubles
    if (H > 0 && W > 0) {
        int wnx, wny;
        bg_max_window(s, wnx, wny);
        if (bg_window_fits(s, wnx, wny)) {
            const int64_t part = nrc_cdiv(W, BG_TX) * nrc_cdiv(H, BG_TY) * wnx * wny * L * 12;
            need = part > need ? part : need;
        }
    }
    return need;
}

int nrc_bilagrid_slice_forward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, int32_t H, int32_t W, int64_t pixel_stride,
                               int64_t channel_stride, int64_t idx, const int32_t* idx_dev, float* out, float* affine, nrc_stream_t stream) {
    NRC_ENTER();
    if (!bg_grid_ok(N, L, Gh, Gw) || !bg_image_ok(H, W) || !grids || !rgb || !out || pixel_stride < 1 || channel_stride < 1) return NRC_ERR_INVALID;
    if (!idx_dev && (idx < 0 || idx >= N)) return NRC_ERR_INVALID;
    if (affine && (reinterpret_cast<uintptr_t>(affine) & 15u)) return NRC_ERR_INVALID;
    if (H == 0 || W == 0) return NRC_OK;
    const BgShape s{L, Gh, Gw, H, W};
    int wnx, wny;
    bg_max_window(s, wnx, wny);
    const dim3 grid((unsigned)nrc_cdiv(W, BG_TX), (unsigned)nrc_cdiv(H, BG_TY));
    hipStream_t st = (hipStream_t)stream;
    NRC_STAGE(st, nullptr);
    if (bg_window_fits(s, wnx, wny))
        hipLaunchKernelGGL(k_bilagrid_slice<true>, grid, dim3(BG_N), 0, st, grids, (int)N, s, rgb, pixel_stride, channel_stride, (int)idx, idx_dev, wnx, wny, out, affine);
    else
        hipLaunchKernelGGL(k_bilagrid_slice<false>, grid, dim3(BG_N), 0, st, grids, (int)N, s, rgb, pixel_stride, channel_stride, (int)idx, idx_dev, wnx, wny, out, affine);
    NRC_STAGE(st, "k_bilagrid_slice");
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_bilagrid_slice_backward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, const float* d_out, int32_t H, int32_t W,
                                int64_t pixel_stride, int64_t channel_stride, int64_t idx, const int32_t* idx_dev, float* workspace, float* d_rgb,
                                float* d_grids, nrc_stream_t stream) {
    NRC_ENTER();
    if (!bg_grid_ok(N, L, Gh, Gw) || !bg_image_ok(H, W) || !grids || !rgb || !d_out || pixel_stride < 1 || channel_stride < 1) return NRC_ERR_INVALID;
    if (!idx_dev && (idx < 0 || idx >= N)) return NRC_ERR_INVALID;
    if (!d_rgb && !d_grids) return NRC_ERR_INVALID;
    if (d_grids && !workspace) return NRC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const BgShape s{L, Gh, Gw, H, W};
    const int64_t E = 12 * (int64_t)L * Gh * Gw;
    if (H == 0 || W == 0) {   // an empty image: the whole grid gradient is zero
        if (d_grids && nrc_zero_async(d_grids, (size_t)(N * E) * 4, st) != hipSuccess) { NRC_LAUNCH_CHECK(); return NRC_ERR_LAUNCH; }
        return NRC_OK;
    }
    int wnx, wny;
    bg_max_window(s, wnx, wny);
    const int ntx = (int)nrc_cdiv(W, BG_TX), nty = (int)nrc_cdiv(H, BG_TY);
    const dim3 grid((unsigned)ntx, (unsigned)nty);
    NRC_STAGE(st, nullptr);
    if (bg_window_fits(s, wnx, wny)) {
        hipLaunchKernelGGL(k_bilagrid_slice_bw<true>, grid, dim3(BG_N), 0, st, grids, (int)N, s, rgb, d_out, pixel_stride, channel_stride, (int)idx, idx_dev, wnx, wny,
                           d_rgb, d_grids ? workspace : (float*)nullptr);
        NRC_STAGE(st, "k_bilagrid_slice_bw");
        if (d_grids)
            hipLaunchKernelGGL(k_bilagrid_reduce, dim3((unsigned)nrc_cdiv(N * E, BG_N)), dim3(BG_N), 0, st, (const float*)workspace, (int)N, s, (int)idx, idx_dev, wnx,
                               wny, ntx, nty, d_grids);
        NRC_STAGE(st, "k_bilagrid_reduce");
    } else {
        if (d_rgb)
            hipLaunchKernelGGL(k_bilagrid_slice_bw<false>, grid, dim3(BG_N), 0, st, grids, (int)N, s, rgb, d_out, pixel_stride, channel_stride, (int)idx, idx_dev, wnx, wny,
                               d_rgb, (float*)nullptr);
        NRC_STAGE(st, "k_bilagrid_slice_bw");
        if (d_grids)
            hipLaunchKernelGGL(k_bilagrid_gather, dim3((unsigned)nrc_cdiv(N * (E / 12), BG_N)), dim3(BG_N), 0, st, (int)N, s, rgb, d_out, pixel_stride, channel_stride,
                               (int)idx, idx_dev, d_grids);
        NRC_STAGE(st, "k_bilagrid_gather");
    }
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_bilagrid_tv_forward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, float* workspace, float* tv, nrc_stream_t stream) {
    NRC_ENTER();
    if (!bg_grid_ok(N, L, Gh, Gw) || !grids || !workspace || !tv || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return NRC_ERR_INVALID;
    const int64_t total = N * 12 * (int64_t)L * Gh * Gw;
    const int blocks = (int)bg_tv_blocks(total);
    const double per = 12.0 * (double)N;
    const double inv_z = L > 1 ? 1.0 / (per * (L - 1) * Gh * Gw) : 0.0, inv_y = Gh > 1 ? 1.0 / (per * L * (Gh - 1) * Gw) : 0.0,
                 inv_x = Gw > 1 ? 1.0 / (per * L * Gh * (Gw - 1)) : 0.0;
    hipStream_t st = (hipStream_t)stream;
    NRC_STAGE(st, nullptr);
    hipLaunchKernelGGL(k_bilagrid_tv, dim3((unsigned)blocks), dim3(BG_N), 0, st, grids, (size_t)total, (int)L, (int)Gh, (int)Gw, reinterpret_cast<double*>(workspace));
    NRC_STAGE(st, "k_bilagrid_tv");
    hipLaunchKernelGGL(k_bilagrid_tv_final, dim3(1), dim3(64), 0, st, reinterpret_cast<const double*>(workspace), blocks, inv_z, inv_y, inv_x, tv);
    NRC_STAGE(st, "k_bilagrid_tv_final");
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

int nrc_bilagrid_tv_backward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, const float* upstream_dev, float* d_grids, nrc_stream_t stream) {
    NRC_ENTER();
    if (!bg_grid_ok(N, L, Gh, Gw) || !grids || !d_grids) return NRC_ERR_INVALID;
    const int64_t total = N * 12 * (int64_t)L * Gh * Gw;
    const double per = 12.0 * (double)N;
    const float kz = L > 1 ? (float)(2.0 / (per * (L - 1) * Gh * Gw)) : 0.f, ky = Gh > 1 ? (float)(2.0 / (per * L * (Gh - 1) * Gw)) : 0.f,
                kx = Gw > 1 ? (float)(2.0 / (per * L * Gh * (Gw - 1))) : 0.f;
    NRC_STAGE((hipStream_t)stream, nullptr);
    hipLaunchKernelGGL(k_bilagrid_tv_bw, dim3((unsigned)nrc_cdiv(total, BG_N)), dim3(BG_N), 0, (hipStream_t)stream, grids, (size_t)total, (int)L, (int)Gh, (int)Gw, kz, ky,
                       kx, upstream_dev, d_grids);
    NRC_STAGE((hipStream_t)stream, "k_bilagrid_tv_bw");
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
