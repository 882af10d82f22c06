// ngp_image_step.h -- the per-sample compositing step of an inference image and its finalisation, shared by every kernel that
// composites the tiled layout (k_composite_image, k_composite_layers in ngp_composite.hip, k_ngp_mlp_composite in ngp_net.hip), so that
// the three paths run the same f32 operation sequence and cannot drift apart: pictures are bit-identical between them by construction.
//
// Reference semantics: volumerendering.cu:205-249 (a ray dies after compositing the sample that brings T <= threshold) and the
// finalisation of render_rays_inference (Renderer.py:133-138).  sigma = exp(h0) (TruncExp), dt re-derived from t with the test
// kernel's step rule (raymarching.cu:370).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

__device__ __forceinline__ float nrc_alpha_of(float sigma, float delta) { return 1.0f - __expf(-sigma * delta); }

// running state of one ray, front to back
struct NrcRayAcc {
    float T, r, g, b, d, o;
    bool alive;
};
__device__ __forceinline__ NrcRayAcc nrc_ray_acc(bool alive) { return NrcRayAcc{1.0f, 0.f, 0.f, 0.f, 0.f, 0.f, alive}; }

// one sample: (h0, r, g, b) as the fp16 values the MLP rounds them to, t its position on the ray; `last` = the ray's final sample.
// Every rounding is spelled out (contraction off, the fused multiply-adds written as such): whether the backend fuses a product into a
// following add otherwise depends on the surrounding kernel -- which vectoriser ran, how often the product is used --, and the kernels that
// share this step must not differ in a single bit.  The sequence is the one the image compositor has always run: the colour sums are
// fused multiply-adds, the depth and opacity sums round the product and the sum separately.
__device__ __forceinline__ void nrc_composite_sample(NrcRayAcc& s, float h0, float cr, float cg, float cb, float t, float esf, float dt_min,
                                                     float dt_max, float thr, bool last) {
#pragma clang fp contract(off)
    const float dt = fmaxf(dt_min, fminf(t * esf, dt_max));
    const float a = nrc_alpha_of(expf(h0), dt);
    const float w = a * s.T;
    s.r = __builtin_fmaf(w, cr, s.r); s.g = __builtin_fmaf(w, cg, s.g); s.b = __builtin_fmaf(w, cb, s.b);
    s.d = s.d + w * t; s.o = s.o + w;
    s.T = s.T * (1.0f - a);
    if (s.T <= thr || last) s.alive = false;
}

// pixel n <- background blend, clamps, inference depth (weighted mean, 0 where nothing was hit)
__device__ __forceinline__ void nrc_composite_finish(const NrcRayAcc& s, float bg_r, float bg_g, float bg_b, int64_t n, float* __restrict__ rgb,
                                                     float* __restrict__ alpha_out, float* __restrict__ depth_out) {
#pragma clang fp contract(off)
    const float al = fminf(fmaxf(s.o, 0.f), 1.f);
    const float Tr = 1.f - al;
    rgb[3 * n] = fminf(fmaxf(__builtin_fmaf(Tr, bg_r, s.r), 0.f), 1.f);
    rgb[3 * n + 1] = fminf(fmaxf(__builtin_fmaf(Tr, bg_g, s.g), 0.f), 1.f);
    rgb[3 * n + 2] = fminf(fmaxf(__builtin_fmaf(Tr, bg_b, s.b), 0.f), 1.f);
    alpha_out[n] = al;
    depth_out[n] = Tr < 1.0f ? s.d / al : 0.0f;
}

// host side: the launch of k_composite_image (ngp_composite.hip), shared by nrc_ngp_composite_image and the full-encoder form of nrc_ngp_render_frame.
// ts: compact rows, or with arena_rows > 0 the count pass's arena; row_capacity 0 = no bound.  The caller checks its arguments and the launch status.
void nrc_launch_composite_image(const void* packed_f16, const float* ts, const int32_t* ray_cnt, const int32_t* tile_off, int32_t width, int32_t height,
                                int64_t tile_begin, int64_t n_tiles, int32_t cascades, float exp_step_factor, int32_t grid_size, int32_t max_samples,
                                float T_threshold, const float* bg3_host, float* rgb, float* alpha, float* depth, int64_t row_capacity, int32_t arena_rows,
                                hipStream_t stream);
