// The optimizer step of optim.hip with every per-step scalar on the device, so that one recorded sequence of launches (a hipGraph of
// the training iteration) stays right when it is replayed, and a loss scaler's verdict never travels to the host: the step count is a
// device float per tensor, the learning rate may be a device float, and the gradient scale and the found-inf flag of
// torch.amp.GradScaler are device floats.  Three kinds of launch beside clip_coef_kernel of optim.hip, which serves both forms
// (clip_coef_dev_kernel is that kernel with max_norm read from the device, for a bound that changes between replays):
//   grad_sqnorm_scaled_kernel   grad_sqnorm_kernel on g / scale: same chunks, same summation order
//   step_advance_kernel         step += 1 unless found_inf, one thread per tensor (the update's workgroups all read the new count,
//                               so no workgroup of the update may be the one that writes it)
//   adamw_capturable_kernel     adamw_kernel, with the scalars of AdamwScalars derived by each workgroup from its item's step count
// A launch whose found_inf is set stores nothing: parameters, moments and step counts keep their bits.
#include "optim_kernels.h"

namespace {

struct StepTable { float* step[HIREST_OPTIM_GROUP_MAX]; int count; };

__device__ __forceinline__ float inv_scale_of(const float* __restrict__ grad_scale) { return grad_scale ? 1.0f / *grad_scale : 1.0f; }

// grad_sqnorm_kernel (optim.hip) on x = g * inv_scale: the squares of the UNSCALED gradients, so that a sum a loss scale of 2^16 would
// push past fp32's range stays where the unscaled one is.  inv_scale = 1 gives grad_sqnorm_kernel's bits.
__global__ __launch_bounds__(THREADS) void grad_sqnorm_scaled_kernel(OptimGroup grp, const float* __restrict__ grad_scale,
                                                                     float* __restrict__ partials) {
    const int i = find_item(grp);
    const hirest_optim_item& it = grp.item[i];
    const int64_t start = (int64_t)((int)blockIdx.x - grp.first[i]) * CHUNK;
    const int n = (int)(it.n - start < CHUNK ? it.n - start : CHUNK);
    const float* __restrict__ g = it.g + start;
    const float inv = inv_scale_of(grad_scale);
    const Split s = split_chunk(g, n);
    const int t = threadIdx.x;
    float a = 0.f;
    const f32x4* gv = reinterpret_cast<const f32x4*>(g + s.head);
#pragma unroll 4
    for (int k = t; k < s.nvec; k += THREADS) {
        const f32x4 x = gv[k] * inv;
        a = __builtin_fmaf(x[0], x[0], a); a = __builtin_fmaf(x[1], x[1], a);
        a = __builtin_fmaf(x[2], x[2], a); a = __builtin_fmaf(x[3], x[3], a);
    }
    if (t < s.head) { const float x = g[t] * inv; a = __builtin_fmaf(x, x, a); }
    if (s.tail0 + t < n) { const float x = g[s.tail0 + t] * inv; a = __builtin_fmaf(x, x, a); }
    a = wave_sum_x(a);
    __shared__ float red[THREADS / 64];
    if ((t & 63) == 0) red[t >> 6] = a;
    __syncthreads();
    if (t == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// step += 1 - found_inf for found_inf in {0, 1} (what GradScaler writes); any other non-zero value skips like 1
__global__ __launch_bounds__(HIREST_OPTIM_GROUP_MAX) void step_advance_kernel(StepTable tab, const float* __restrict__ found_inf) {
    const int i = threadIdx.x;
    if (i >= tab.count) return;
    if (found_inf && *found_inf != 0.f) return;
    *tab.step[i] += 1.0f;
}

// clip_coef_kernel (optim.hip) with max_norm in device memory: the same sums in the same order
__global__ __launch_bounds__(THREADS) void clip_coef_dev_kernel(const float* __restrict__ partials, int64_t n,
                                                                const float* __restrict__ max_norm, float* __restrict__ out) {
    const double sum = sum_partials(partials, n);
    if (threadIdx.x == 0) write_norm_coef(sum, *max_norm, out);
}

struct CapturableArgs {
    const float* coef;          // clip coefficient; NULL = 1
    const float* lr_ptr;        // learning rate on the device; NULL = lr below
    const float* grad_scale;    // NULL = 1
    const float* found_inf;     // NULL = 0
    double lr, beta1, beta2, weight_decay;
    float eps;
};

// adamw_kernel (optim.hip) on g * inv_scale.  The scalars are optim.hyperparameters' expressions in double from the item's step count
// (already advanced) and the learning rate, rounded to fp32 as the host's are when they enter adamw_kernel's arguments.  All inputs
// are uniform over the workgroup; the double pow costs a few hundred instructions per wave against 224 KB of traffic per chunk.
__global__ __launch_bounds__(THREADS) void adamw_capturable_kernel(OptimGroup grp, StepTable tab, CapturableArgs a) {
    if (a.found_inf && *a.found_inf != 0.f) return;
    const int i = find_item(grp);
    const hirest_optim_item& it = grp.item[i];
    const int64_t start = (int64_t)((int)blockIdx.x - grp.first[i]) * CHUNK;
    const int n = (int)(it.n - start < CHUNK ? it.n - start : CHUNK);
    float* __restrict__ p = it.p + start;
    const float* __restrict__ g = it.g + start;
    float* __restrict__ m = it.m + start;
    float* __restrict__ v = it.v + start;
    const float coef = a.coef ? *a.coef : 1.0f;
    const float inv = inv_scale_of(a.grad_scale);
    const double t_step = (double)*tab.step[i];
    const double lr = a.lr_ptr ? (double)*a.lr_ptr : a.lr;
    const double bc1 = 1.0 - pow(a.beta1, t_step), bc2 = 1.0 - pow(a.beta2, t_step);
    const AdamwScalars h{(float)(1.0 - lr * a.weight_decay), (float)(1.0 - a.beta1), (float)a.beta2, (float)(1.0 - a.beta2),
                         (float)(lr / bc1), (float)sqrt(bc2), a.eps};
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
            adamw_one(p1, gg[c] * inv, m1, v1, coef, h);
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
            adamw_one(pp, g[e] * inv, mm, vv, coef, h);
            p[e] = pp; m[e] = mm; v[e] = vv;
        }
    }
}

// the step pointers of a launch; false when the table is unusable
inline bool fill_steps(float* const* steps, int32_t count, StepTable* t) {
    if (!steps || count <= 0 || count > HIREST_OPTIM_GROUP_MAX) return false;
    for (int i = 0; i < count; ++i) {
        if (!steps[i]) return false;
        t->step[i] = steps[i];
    }
    t->count = count;
    return true;
}

}  // namespace

#define S_(stream) reinterpret_cast<hipStream_t>(stream)

extern "C" int hirest_grad_sqnorm_scaled_grouped_f32(const hirest_optim_item* items, int32_t count, const float* grad_scale,
                                                     float* partials, void* stream) {
    if (!partials) return HIREST_E_BADARG;
    OptimGroup g;
    const int64_t blocks = fill_group(items, count, false, &g);
    if (blocks < 0) return blocks == -2 ? HIREST_E_SHAPE : HIREST_E_BADARG;
    hipLaunchKernelGGL(grad_sqnorm_scaled_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, S_(stream), g, grad_scale, partials);
    return hirest_launch_status();
}

extern "C" int hirest_clip_coef_dev_f32(const float* partials, int64_t count, const float* max_norm, float* norm_coef, void* stream) {
    if (!partials || !max_norm || !norm_coef || count <= 0) return HIREST_E_BADARG;
    hipLaunchKernelGGL(clip_coef_dev_kernel, dim3(1), dim3(THREADS), 0, S_(stream), partials, count, max_norm, norm_coef);
    return hirest_launch_status();
}

extern "C" int hirest_optim_step_advance_f32(float* const* steps, int32_t count, const float* found_inf, void* stream) {
    StepTable t;
    if (!fill_steps(steps, count, &t)) return HIREST_E_BADARG;
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(HIREST_OPTIM_GROUP_MAX), 0, S_(stream), t, found_inf);
    return hirest_launch_status();
}

extern "C" int hirest_adamw_capturable_grouped_f32(const hirest_optim_item* items, float* const* steps, int32_t count, const float* coef,
                                                   const float* lr_ptr, double lr, const float* grad_scale, const float* found_inf,
                                                   double beta1, double beta2, float eps, double weight_decay, void* stream) {
    OptimGroup g;
    StepTable t;
    const int64_t blocks = fill_group(items, count, true, &g);
    if (blocks < 0) return blocks == -2 ? HIREST_E_SHAPE : HIREST_E_BADARG;
    if (!fill_steps(steps, count, &t)) return HIREST_E_BADARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return HIREST_E_BADARG;
    const CapturableArgs a{coef, lr_ptr, grad_scale, found_inf, lr, beta1, beta2, weight_decay, eps};
    hipLaunchKernelGGL(adamw_capturable_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, S_(stream), g, t, a);
    return hirest_launch_status();
}
