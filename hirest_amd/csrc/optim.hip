// Optimizer step of the joint model's training loop (run.py:264-295, trainer_base.py:55-61): clip_grad_norm_ followed
// by torch.optim.AdamW, as three kinds of launch — per-chunk sums of squared gradients, one block that turns them into the total
// norm and the clip coefficient (both stay on the device), and the update itself, which reads p, g, m, v once and writes p, m, v
// once (28 B per element) with the coefficient applied to g on the fly.  fp32, streaming, memory-bound: plain C++ with 16-byte
// loads and stores, no LDS beyond the block reductions.
//
// Work is a table of items (one per parameter tensor) that travels in the kernel arguments like ColsumGroup of train.hip: gradient
// pointers change every step (the loop sets param.grad = None), so a device-resident table would need a copy per step.  Item i
// owns ceil(n_i / HIREST_OPTIM_CHUNK) consecutive blocks; a block works on one chunk of one tensor and never crosses into the next.
#include "optim_kernels.h"

namespace {

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
    const double sum = sum_partials(partials, n);
    if (threadIdx.x == 0) write_norm_coef(sum, max_norm, out);
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
