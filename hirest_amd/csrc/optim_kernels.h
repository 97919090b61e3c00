// Shared pieces of the optimizer kernels (optim.hip: the step with host-derived scalars; optim_capturable.hip: the step whose
// scalars live on the device): the item table in the kernel arguments, the chunk a workgroup owns, the head / body / tail split
// and AdamW's arithmetic for one element.
#pragma once
#include "common.h"

namespace {

constexpr int CHUNK = HIREST_OPTIM_CHUNK;
constexpr int THREADS = 256;

struct OptimGroup { hirest_optim_item item[HIREST_OPTIM_GROUP_MAX]; int first[HIREST_OPTIM_GROUP_MAX]; int count; };

// AdamW's scalars of one update, all derived in double (torch's _single_tensor_adam with capturable = False): by the host for a whole
// launch of optim.hip, by each workgroup from its item's device step count in optim_capturable.hip
struct AdamwScalars {
    float decay;            // 1 - lr * weight_decay
    float w1;               // 1 - beta1 (the lerp weight)
    float beta2, w2;        // beta2, 1 - beta2
    float step_size;        // lr / (1 - beta1^t)
    float bc2_sqrt;         // sqrt(1 - beta2^t)
    float eps;
};

// which chunk of which item this block owns: first[] ascends, so the item is the number of later items starting at or before this block
// (independent scalar loads, as in weighted_colsum_grouped_kernel)
__device__ __forceinline__ int find_item(const OptimGroup& g) {
    int i = 0;
#pragma unroll
    for (int j = 1; j < HIREST_OPTIM_GROUP_MAX; ++j) i += (j < g.count && (int)blockIdx.x >= g.first[j]) ? 1 : 0;
    return i;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// a 16-byte access where the address allows it, four 4-byte ones otherwise (`vec` is uniform over the block: no divergence)
__device__ __forceinline__ f32x4 load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(p);
    return f32x4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void store4(float* p, bool vec, const f32x4& x) {
    if (vec) { *reinterpret_cast<f32x4*>(p) = x; return; }
    p[0] = x[0]; p[1] = x[1]; p[2] = x[2]; p[3] = x[3];
}

// A chunk [0, n) that starts `lead` elements (0..3) before a 16-byte boundary of its leading pointer splits into a scalar head of
// `head` elements, `nvec` float4 and a scalar tail; the split depends on the pointer's phase alone, which is the same for every
// chunk of a tensor (CHUNK is a multiple of 4).
struct Split { int head, nvec, tail0; };
__device__ __forceinline__ Split split_chunk(const float* lead, int n) {
    int head = (int)((16 - (reinterpret_cast<uintptr_t>(lead) & 15)) & 15) >> 2;
    head = head < n ? head : n;
    const int nvec = (n - head) >> 2;
    return {head, nvec, head + 4 * nvec};
}

// The sum of n partials over one block, valid in thread 0: thread t adds partials t, t + 256, ... in index order, then a fixed tree over
// the threads, all in double.
__device__ __forceinline__ double sum_partials(const float* __restrict__ partials, int64_t n) {
    __shared__ double red[THREADS];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int64_t k = t; k < n; k += THREADS) a += (double)partials[k];
    red[t] = a;
    __syncthreads();
#pragma unroll
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ void write_norm_coef(double sum, float max_norm, float* __restrict__ out) {
    const float norm = (float)sqrt(sum);
    out[0] = norm;
    out[1] = fminf(1.0f, max_norm / (norm + 1e-6f));
}

// torch.optim.AdamW, one element: the operations of _single_tensor_adam (capturable = False) in its order, on g' = coef * g
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float coef, const AdamwScalars& h) {
    g *= coef;                                               // clip_grad_norm_: g.mul_(coef)
    p *= h.decay;                                            // param.mul_(1 - lr * weight_decay)
    m = m + h.w1 * (g - m);                                  // exp_avg.lerp_(grad, 1 - beta1)
    v = v * h.beta2 + h.w2 * g * g;                          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;       // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - h.step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// blocks of a group and their first-block numbers; < 0 when the table is unusable
inline int64_t fill_group(const hirest_optim_item* items, int32_t count, bool update, OptimGroup* g) {
    if (!items || count <= 0 || count > HIREST_OPTIM_GROUP_MAX) return -1;
    int64_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        const hirest_optim_item& it = items[i];
        if (!it.g || it.n <= 0 || (update && (!it.p || !it.m || !it.v))) return -1;
        if (g) { g->item[i] = it; g->first[i] = (int)blocks; }
        blocks += (it.n + CHUNK - 1) / CHUNK;
        if (blocks > INT32_MAX) return -2;
    }
    if (g) g->count = count;
    return blocks;
}

}  // namespace
