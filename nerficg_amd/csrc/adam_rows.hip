// adam_rows.hip -- the visibility-masked Adam step of the 3DGS model (include/nerficg_hip.h group 24): every tensor of the call is (n_rows, width) f32 and
// shares ONE row mask (the rasterizer's radii, or a byte mask).  A visible row gets the update of adam_math.h, the one statement of the arithmetic that the
// dense step uses as well (no FMA contraction here either: the two steps leave the same bits); an invisible row keeps parameter and both moments bit for
// bit, whatever its gradient holds -- the step of Taming-3DGS / 3DGS `sparse_adam` / gsplat `SelectiveAdam`, with this project's operation order.
// Pure HBM streaming like the dense step, 28 B per element of a visible row; the point of the mask is the traffic that does NOT happen: a work item whose
// four elements all lie in invisible rows issues no load and no store of p, g, m or v.  HBM moves 128-B lines, so bytes are saved where all eight work
// items of a line are invisible -- common in the 180-B f_rest rows (45 of the model's 59 floats per Gaussian), rare in the 4..16-B rows unless visibility
// is spatially coherent.
#include <hip/hip_runtime.h>

#include "common.h"
#include "adam_math.h"

namespace {

#define ADAM_ROWS_MAX 12
struct RowTensor { float* p; const float* g; float* m; float* v; int64_t n; float lr, bc1, bc2; int block0; int32_t width; };
struct RowList { RowTensor t[ADAM_ROWS_MAX]; int n; };

// KIND 0: bytes, non-zero = visible.  KIND 1: int32 radii, > 0 = visible.
template <int KIND>
__device__ __forceinline__ bool row_visible(const void* __restrict__ mask, int64_t row) {
    if constexpr (KIND == 0) return static_cast<const uint8_t*>(mask)[row] != 0;
    else return static_cast<const int32_t*>(mask)[row] > 0;
}

// Four consecutive elements starting at i0 (a multiple of 4, < n).  The visibility of element i is mask[i / width]: ONE division per work item (32-bit
// where the tensor has fewer than 2^31 elements, which the caller's SMALL says; 64-bit otherwise), the three following elements walk the remainder.
// Widths >= 4 put the four elements into at most two rows (those of the first and of the last element): two mask loads; narrower rows load per element.
// Elements past n count as invisible and are never touched.
template <bool ALIGNED, int KIND, bool SMALL>
__device__ __forceinline__ void adam_rows_four(const RowTensor& t, const void* __restrict__ mask, int64_t i0, const NrcAdamHyper& h) {
    const int32_t w = t.width;
    int64_t row0;
    int32_t rem0;
    if constexpr (SMALL) {
        const uint32_t q = (uint32_t)i0 / (uint32_t)w;
        row0 = q; rem0 = (int32_t)((uint32_t)i0 - q * (uint32_t)w);
    } else {
        row0 = i0 / w; rem0 = (int32_t)(i0 - row0 * w);
    }
    const int count = t.n - i0 < 4 ? (int)(t.n - i0) : 4;   // elements of this work item inside the tensor (1..4)
    int64_t row[4];
    {
        int64_t r = row0; int32_t rem = rem0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            row[k] = r;
            if (++rem == w) { rem = 0; r++; }
        }
    }
    bool vis[4];
    if (w >= 4) {   // uniform per tensor
        const bool first = row_visible<KIND>(mask, row0);
        int64_t row_last = row0;
#pragma unroll
        for (int k = 1; k < 4; k++) row_last = k < count ? row[k] : row_last;
        const bool last = row_last != row0 ? row_visible<KIND>(mask, row_last) : first;
#pragma unroll
        for (int k = 0; k < 4; k++) vis[k] = k < count && (row[k] == row0 ? first : last);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) vis[k] = k < count && row_visible<KIND>(mask, row[k]);
    }
    if (!(vis[0] || vis[1] || vis[2] || vis[3])) return;   // nothing of this work item is visible: no access to p, g, m, v at all

    float* __restrict__ p = t.p; const float* __restrict__ g = t.g; float* __restrict__ m = t.m; float* __restrict__ v = t.v;
    if (ALIGNED && count == 4) {   // 16-byte access; elements of invisible rows go back as they came
        float pv[4], gv[4], mv[4], vv[4];
        *reinterpret_cast<float4*>(pv) = *reinterpret_cast<const float4*>(p + i0);
        *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(g + i0);
        *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m + i0);
        *reinterpret_cast<float4*>(vv) = *reinterpret_cast<const float4*>(v + i0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float pk = pv[k], mk = mv[k], vk = vv[k];
            nrc_adam_update(pk, gv[k], mk, vk, h, false, 0.f);
            pv[k] = vis[k] ? pk : pv[k]; mv[k] = vis[k] ? mk : mv[k]; vv[k] = vis[k] ? vk : vv[k];
        }
        *reinterpret_cast<float4*>(p + i0) = *reinterpret_cast<const float4*>(pv);
        *reinterpret_cast<float4*>(m + i0) = *reinterpret_cast<const float4*>(mv);
        *reinterpret_cast<float4*>(v + i0) = *reinterpret_cast<const float4*>(vv);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!vis[k]) continue;
            float pk = p[i0 + k], mk = m[i0 + k], vk = v[i0 + k];
            nrc_adam_update(pk, g[i0 + k], mk, vk, h, false, 0.f);
            p[i0 + k] = pk; m[i0 + k] = mk; v[i0 + k] = vk;
        }
    }
}

// all tensors of the call in ONE launch: block0 ascending, a workgroup belongs to the last tensor that starts at or before it
template <int KIND>
__global__ void __launch_bounds__(256) k_adam_rows(RowList l, const void* __restrict__ mask, float beta1, float beta2, float eps, float weight_decay, int adam_w_mode) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < ADAM_ROWS_MAX; q++) k += (q < l.n && (int)blockIdx.x >= l.t[q].block0) ? 1 : 0;
    const RowTensor t = l.t[k];
    const int64_t i0 = ((int64_t)((int)blockIdx.x - t.block0) * 256 + threadIdx.x) * 4;
    if (i0 >= t.n) return;
    const NrcAdamHyper h{t.lr, beta1, beta2, eps, weight_decay, adam_w_mode, t.bc1, t.bc2, 1.0f};
    const bool aligned = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15u) == 0);   // uniform per tensor
    const bool small = t.n < ((int64_t)1 << 31);                                                                  // uniform per tensor
    if (aligned) {
        if (small) adam_rows_four<true, KIND, true>(t, mask, i0, h);
        else adam_rows_four<true, KIND, false>(t, mask, i0, h);
    } else {
        if (small) adam_rows_four<false, KIND, true>(t, mask, i0, h);
        else adam_rows_four<false, KIND, false>(t, mask, i0, h);
    }
}

}  // namespace

extern "C" {

int nrc_adam_step_rows_multi(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                             const int32_t* row_widths, int64_t n_rows, const void* visible, int32_t visible_kind, const float* lrs, const float* bc1,
                             const float* bc2, float beta1, float beta2, float eps, float weight_decay, int32_t adam_w_mode, nrc_stream_t stream) {
    // every argument is judged before the first HIP call
    if (n_tensors < 1 || n_tensors > ADAM_ROWS_MAX || n_rows < 0 || (visible_kind != 0 && visible_kind != 1)) return NRC_ERR_INVALID;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !row_widths || !visible || !lrs || !bc1 || !bc2) return NRC_ERR_INVALID;
    RowList l;
    l.n = 0;
    int64_t blocks = 0;
    for (int k = 0; k < n_tensors; k++) {
        if (row_widths[k] <= 0 || !(bc1[k] > 0.f) || !(bc2[k] > 0.f)) return NRC_ERR_INVALID;
        if (n_rows == 0) continue;
        if (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k]) return NRC_ERR_INVALID;
        if (n_rows > INT64_MAX / row_widths[k]) return NRC_ERR_INVALID;
        const int64_t n = n_rows * row_widths[k];
        l.t[l.n++] = RowTensor{params[k], grads[k], exp_avg[k], exp_avg_sq[k], n, lrs[k], bc1[k], bc2[k], (int)blocks, row_widths[k]};
        blocks += nrc_cdiv(nrc_cdiv(n, 4), 256);
        if (blocks > 0x7fffffff) return NRC_ERR_INVALID;
    }
    if (l.n == 0) return NRC_OK;
    for (int k = l.n; k < ADAM_ROWS_MAX; k++) l.t[k] = RowTensor{nullptr, nullptr, nullptr, nullptr, 0, 0.f, 1.f, 1.f, 0x7fffffff, 1};
    NRC_ENTER();
    if (visible_kind == 0)
        hipLaunchKernelGGL(k_adam_rows<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, l, visible, beta1, beta2, eps, weight_decay, (int)adam_w_mode);
    else
        hipLaunchKernelGGL(k_adam_rows<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, l, visible, beta1, beta2, eps, weight_decay, (int)adam_w_mode);
    NRC_LAUNCH_CHECK();
    return NRC_OK;
}

}  // extern "C"
