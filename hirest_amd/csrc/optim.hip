// Optimizer step of the joint model's training loop (run.py:264-295, trainer_base.py:55-61): clip_grad_norm_ followed
// by torch.optim.AdamW, as three kinds of launch — per-chunk sums of squared gradients, one block that turns them into the total
// norm and the clip coefficient (both stay on the device), and the update itself, which reads p, g, m, v once and writes p, m, v
// once (28 B per element) with the coefficient applied to g on the fly.  fp32, streaming, memory-bound: plain C++ with 16-byte
// loads and stores, no LDS beyond the block reductions.
//
// Work is a table of items (one per parameter tensor) that travels in the kernel arguments like ColsumGroup of train.hip: gradient
// pointers change every step (the loop sets param.grad = None), so a device-resident table would need a copy per step.  Item i
// owns ceil(n_i / HIREST_OPTIM_CHUNK) consecutive blocks; a block works on one chunk of one tensor and never crosses into the next.
#include "common.h"

namespace {

constexpr int CHUNK = HIREST_OPTIM_CHUNK;
constexpr int THREADS = 256;

struct OptimGroup { hirest_optim_item item[HIREST_OPTIM_GROUP_MAX]; int first[HIREST_OPTIM_GROUP_MAX]; int count; };

// AdamW's scalars of one launch, all derived on the host in double (torch's _single_tensor_adam with capturable = False)
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

// partial[block] = sum of g^2 over the block's chunk.  Fixed order: a thread adds its float4 (element 0..3 in turn) in ascending
// address order, then at most one head and one tail element; the 64 lanes of a wave and then the four waves are added in a fixed
// tree.  No atomics: the same gradients at the same addresses give the same bits.
__global__ __launch_bounds__(THREADS) void grad_sqnorm_kernel(OptimGroup grp, float* __restrict__ partials) {
    const int i = find_item(grp);
    const hirest_optim_item& it = grp.item[i];
    const int64_t start = (int64_t)((int)blockIdx.x - grp.first[i]) * CHUNK;
    const int n = (int)(it.n - start < CHUNK ? it.n - start : CHUNK);
    const float* __restrict__ g = it.g + start;
    const Split s = split_chunk(g, n);
    const int t = threadIdx.x;
    float a = 0.f;
    const f32x4* gv = reinterpret_cast<const f32x4*>(g + s.head);
#pragma unroll 4
    for (int k = t; k < s.nvec; k += THREADS) {
        const f32x4 x = gv[k];
        a = __builtin_fmaf(x[0], x[0], a); a = __builtin_fmaf(x[1], x[1], a);
        a = __builtin_fmaf(x[2], x[2], a); a = __builtin_fmaf(x[3], x[3], a);
    }
    if (t < s.head) a = __builtin_fmaf(g[t], g[t], a);
    if (s.tail0 + t < n) a = __builtin_fmaf(g[s.tail0 + t], g[s.tail0 + t], a);
    a = wave_sum_x(a);
    __shared__ float red[THREADS / 64];
    if ((t & 63) == 0) red[t >> 6] = a;
    __syncthreads();
    if (t == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = total_norm = sqrt(sum of the partials), out[1] = coef = min(1, max_norm / (total_norm + 1e-6)): clip_grad_norm_'s rule
// with error_if_nonfinite = False.  One block: thread t adds partials t, t + 256, ... in index order, then a fixed tree over the
// threads.  The few thousand partials are added in double (free here), so the sum's error is that of the chunks alone.
__global__ __launch_bounds__(THREADS) void clip_coef_kernel(const float* __restrict__ partials, int64_t n, float max_norm,
                                                            float* __restrict__ out) {
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
    if (t == 0) {
        const float norm = (float)sqrt(red[0]);
        out[0] = norm;
        out[1] = fminf(1.0f, max_norm / (norm + 1e-6f));
    }
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

// g is read and never written.  The head / body / tail split follows p (its loads and stores are always 16 bytes wide in the body);
// g, m and v use 16-byte accesses when they share p's phase and 4-byte ones otherwise (a parameter that is a view at an odd offset
// has freshly allocated, aligned moments).
__global__ __launch_bounds__(THREADS) void adamw_kernel(OptimGroup grp, const float* __restrict__ coef_ptr, AdamwScalars h) {
    const int i = find_item(grp);
    const hirest_optim_item& it = grp.item[i];
    const int64_t start = (int64_t)((int)blockIdx.x - grp.first[i]) * CHUNK;
    const int n = (int)(it.n - start < CHUNK ? it.n - start : CHUNK);
    float* __restrict__ p = it.p + start;
    const float* __restrict__ g = it.g + start;
    float* __restrict__ m = it.m + start;
    float* __restrict__ v = it.v + start;
    const float coef = coef_ptr ? *coef_ptr : 1.0f;
    const Split s = split_chunk(p, n);
    const bool gvec = aligned16(g + s.head), mvec = aligned16(m + s.head), vvec = aligned16(v + s.head);
    const int t = threadIdx.x;
#pragma unroll 2
    for (int k = t; k < s.nvec; k += THREADS) {
        const int e = s.head + 4 * k;
        f32x4 pp = *reinterpret_cast<const f32x4*>(p + e);
        const f32x4 gg = load4(g + e, gvec);
        f32x4 mm = load4(m + e, mvec), vv = load4(v + e, vvec);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float p1 = pp[c], m1 = mm[c], v1 = vv[c];
            adamw_one(p1, gg[c], m1, v1, coef, h);
            pp[c] = p1; mm[c] = m1; vv[c] = v1;
        }
        *reinterpret_cast<f32x4*>(p + e) = pp;
        store4(m + e, mvec, mm);
        store4(v + e, vvec, vv);
    }
    // head (threads 0 .. head-1) and tail (threads 0 .. n - tail0 - 1): at most three elements each
    for (int pass = 0; pass < 2; ++pass) {
        const int e = pass == 0 ? t : s.tail0 + t;
        const int end = pass == 0 ? s.head : n;
        if (e < end) {
            float pp = p[e], mm = m[e], vv = v[e];
            adamw_one(pp, g[e], mm, vv, coef, h);
            p[e] = pp; m[e] = mm; v[e] = vv;
        }
    }
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

#define S_(stream) reinterpret_cast<hipStream_t>(stream)

extern "C" int64_t hirest_optim_partials_count(const hirest_optim_item* items, int32_t count) {
    const int64_t blocks = fill_group(items, count, false, nullptr);
    return blocks == -2 ? HIREST_E_SHAPE : blocks < 0 ? HIREST_E_BADARG : blocks;
}

extern "C" int hirest_grad_sqnorm_grouped_f32(const hirest_optim_item* items, int32_t count, float* partials, void* stream) {
    if (!partials) return HIREST_E_BADARG;
    OptimGroup g;
    const int64_t blocks = fill_group(items, count, false, &g);
    if (blocks < 0) return blocks == -2 ? HIREST_E_SHAPE : HIREST_E_BADARG;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, S_(stream), g, partials);
    return hirest_launch_status();
}

extern "C" int hirest_clip_coef_f32(const float* partials, int64_t count, float max_norm, float* norm_coef, void* stream) {
    if (!partials || !norm_coef || count <= 0) return HIREST_E_BADARG;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(THREADS), 0, S_(stream), partials, count, max_norm, norm_coef);
    return hirest_launch_status();
}

extern "C" int hirest_adamw_grouped_f32(const hirest_optim_item* items, int32_t count, const float* coef, float decay,
                                        float one_minus_beta1, float beta2, float one_minus_beta2, float step_size, float bc2_sqrt,
                                        float eps, void* stream) {
    OptimGroup g;
    const int64_t blocks = fill_group(items, count, true, &g);
    if (blocks < 0) return blocks == -2 ? HIREST_E_SHAPE : HIREST_E_BADARG;
    if (!(bc2_sqrt > 0.f)) return HIREST_E_BADARG;
    const AdamwScalars h{decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps};
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, S_(stream), g, coef, h);
    return hirest_launch_status();
}
