// The seams of the end-to-end cascade (run.py:383-490): what the reference does between its three stages by rewriting
// all_data_test.json and rebuilding the dataset from it (hirest_dataset.py:186-311), as three small device steps, so that the
// predictions of one stage become the inputs of the next without leaving the GPU.  Integer / index work and one row gather:
// no MFMA.  Timestamps go through the double-precision bins of timeline_bins.h, so every integer is the reference's.
#include "common.h"
#include "timeline_bins.h"

namespace {

// ---- (a) moment retrieval -> moment segmentation.  One workgroup per sample: run.py:731-732 (frames -> seconds),
// hirest_dataset.py:250-261 (seconds -> frames again, moment_mask[s : e + 1] = 1), modeling.py:376-382 (boundary mask).
__global__ void moment_bounds_kernel(const int32_t* __restrict__ pred, const double* __restrict__ duration,
                                     const int32_t* __restrict__ n_frames, int32_t n_frames_all, int T,
                                     int64_t* __restrict__ bounds_ts, int32_t* __restrict__ bound_frames,
                                     int32_t* __restrict__ moment_mask, int32_t* __restrict__ boundary_mask) {
    const int b = blockIdx.x;
    Bins bins;
    int64_t ts0 = INT64_MIN, ts1 = INT64_MIN;
    int s = -1, e = -1;
    if (make_bins(duration[b], n_frames ? n_frames[b] : n_frames_all, bins)) {
        ts0 = bins_frame_to_timestamp(bins, pred[2 * b]);
        ts1 = bins_frame_to_timestamp(bins, pred[2 * b + 1]);
        if (ts0 != INT64_MIN && ts1 != INT64_MIN) {
            s = (int)bins_timestamp_to_frame(bins, (double)ts0);
            e = (int)bins_timestamp_to_frame(bins, (double)ts1);
        }
    }
    if (threadIdx.x == 0) {
        bounds_ts[2 * b] = ts0; bounds_ts[2 * b + 1] = ts1;
        bound_frames[2 * b] = s; bound_frames[2 * b + 1] = e;
    }
    for (int t = threadIdx.x; t < T; t += blockDim.x) {          // Python slice [s : e + 1]: empty when s > e
        moment_mask[(int64_t)b * T + t] = (s >= 0 && t >= s && t <= e) ? 1 : 0;
        boundary_mask[(int64_t)b * T + t] = (t == s) ? 1 : 0;
    }
}

// ---- (b) segmentation -> steps, part 1.  One wave per sample: the list post-processing of modeling.py:435-463 on at most 64 values.
constexpr int CAP_MAX = 64;
__global__ void __launch_bounds__(256) boundaries_kernel(const int32_t* __restrict__ steps, const int32_t* __restrict__ nsteps,
                                                         const int32_t* __restrict__ bound_frames, int B, int iters, int cap,
                                                         int32_t* __restrict__ n_bounds, int32_t* __restrict__ bounds) {
    __shared__ int32_t flat_s[4][CAP_MAX];
    __shared__ int32_t uniq_s[4][CAP_MAX];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + w;
    if (b >= B) return;                                          // wave-uniform; no workgroup barrier below
    int32_t* flat = flat_s[w];
    int32_t* uniq = uniq_s[w];
    const int s = bound_frames[2 * b], l = bound_frames[2 * b + 1];
    int ns = nsteps[b];
    ns = ns < 0 ? 0 : (ns > iters ? iters : ns);
    const int np = ns + 2;                                       // pairs: [s, s], the steps in the order they were found, [l, l]
    int p0 = 0, p1 = 0;
    if (lane < np) {
        if (lane == 0) { p0 = s; p1 = s; }
        else if (lane == np - 1) { p0 = l; p1 = l; }
        else { p0 = steps[((int64_t)b * iters + (lane - 1)) * 2]; p1 = steps[((int64_t)b * iters + (lane - 1)) * 2 + 1]; }
    }
    // list.sort(key = first element) is stable: the rank of pair i counts the pairs with a smaller key, and the earlier ones of equal key
    int rank = 0;
    for (int j = 0; j < np; ++j) {
        const int k = __shfl(p0, j, 64);
        rank += (k < p0 || (k == p0 && j < lane)) ? 1 : 0;
    }
    if (lane < np) { flat[2 * rank] = p0; flat[2 * rank + 1] = p1; }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int n = 2 * np;
    const int v = lane < n ? flat[lane] : 0;
    // while flat[-1] > l: pop  -> keep up to the last value that is <= l (the [l, l] pair guarantees one)
    const unsigned long long le = __ballot(lane < n && v <= l);
    const int m = le ? 64 - __builtin_clzll(le) : 0;
    // sorted(set(.)): a value's first occurrence goes to the number of distinct smaller values
    bool first = lane < m;
    for (int j = 0; j < m; ++j) {
        const int vj = __shfl(v, j, 64);
        if (j < lane && vj == v) first = false;
    }
    const unsigned long long fm = __ballot(first);
    int pos = 0;
    for (int j = 0; j < m; ++j) {
        const int vj = __shfl(v, j, 64);
        pos += (((fm >> j) & 1ull) && vj < v) ? 1 : 0;
    }
    if (first) uniq[pos] = v;
    const int nu = __popcll(fm);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // keep the first value, then every interior one at least 5 frames after the last kept; the final value is never kept
    if (lane == 0) {
        int32_t* o = bounds + (int64_t)b * cap;
        int cnt = 0;
        if (nu > 0) {
            int cur = uniq[0];
            o[cnt++] = cur;
            for (int i = 1; i < nu - 1; ++i)
                if (uniq[i] - cur >= 5) { cur = uniq[i]; o[cnt++] = cur; }
        }
        n_bounds[b] = cnt;
        for (int i = cnt; i < cap; ++i) o[i] = -1;
    }
}

// ---- (b) part 2.  One wave per sample: its offset among all steps (a fixed-order integer sum over the samples before it), then the
// consecutive boundary pairs as timestamps (run.py:766-770) and as the frames the captioning dataset derives from those
// (hirest_dataset.py:289-290).
__global__ void __launch_bounds__(256) steps_kernel(const int32_t* __restrict__ n_bounds, const int32_t* __restrict__ bounds,
                                                    const double* __restrict__ duration, const int32_t* __restrict__ n_frames,
                                                    int32_t n_frames_all, int B, int cap, int64_t* __restrict__ step_ts,
                                                    int32_t* __restrict__ step_frames, int32_t* __restrict__ step_sample,
                                                    int32_t* __restrict__ offsets) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int off = 0;
    for (int j = lane; j < b; j += 64) { const int nb = n_bounds[j]; off += nb > 1 ? nb - 1 : 0; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    const int nb = n_bounds[b];
    const int mine = nb > 1 ? nb - 1 : 0;
    if (lane == 0) {
        offsets[b] = off;
        if (b == B - 1) offsets[B] = off + mine;
    }
    if (lane >= mine) return;
    Bins bins;
    const bool ok = make_bins(duration[b], n_frames ? n_frames[b] : n_frames_all, bins);
    const int64_t r = (int64_t)off + lane;
    for (int k = 0; k < 2; ++k) {
        const int64_t ts = ok ? bins_frame_to_timestamp(bins, bounds[(int64_t)b * cap + lane + k]) : INT64_MIN;
        step_ts[2 * r + k] = ts;
        step_frames[2 * r + k] = (ok && ts != INT64_MIN) ? (int32_t)bins_timestamp_to_frame(bins, (double)ts) : -1;
    }
    step_sample[r] = b;
}

// ---- (c) steps -> decoder inputs.  trim_feats (modeling.py:529-554) of the captioning mask `mask[a:e] = 1; mask[e] = 1`
// (hirest_dataset.py:302-304), whose selected frames are a contiguous range: one wave copies one output row.
__global__ void __launch_bounds__(256) trim_gather_kernel(const float* __restrict__ vis, const float* __restrict__ asr,
                                                          const int32_t* __restrict__ step_frames, const int32_t* __restrict__ step_sample,
                                                          int64_t rows, int B, int T, int D, int Da, int F,
                                                          float* __restrict__ out_vis, float* __restrict__ out_asr) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t s = r / F;
    const int p = (int)(r - s * F);
    const int a = step_frames[2 * s], e = step_frames[2 * s + 1], smp = step_sample[s];
    const int first = a <= e ? a : e;                           // a > e: the slice is empty and mask[e] alone is set
    const int N = a <= e ? e - a + 1 : 1;
    const int j = N > F ? p : ((p + 1) * N + F - 1) / F - 1;    // more frames than slots: the first F; else frame j repeated
    const int t = first + j;
    const bool ok = smp >= 0 && smp < B && a >= 0 && e >= 0 && e < T;   // then first + j <= e: inside the sample's rows
    const int64_t src = ok ? (int64_t)smp * T + t : 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4* vi = reinterpret_cast<const f32x4*>(vis + src * D);
    f32x4* vo = reinterpret_cast<f32x4*>(out_vis + r * D);
    for (int i = lane; i < D / 4; i += 64) vo[i] = ok ? vi[i] : zero;
    if (asr) {
        const f32x4* ai = reinterpret_cast<const f32x4*>(asr + src * Da);
        f32x4* ao = reinterpret_cast<f32x4*>(out_asr + r * Da);
        for (int i = lane; i < Da / 4; i += 64) ao[i] = ok ? ai[i] : zero;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int hirest_cascade_moment_bounds(const int32_t* pred_frames, const double* duration, const int32_t* n_frames,
                                            int32_t n_frames_all, int32_t B, int32_t T, int64_t* bounds_ts, int32_t* bound_frames,
                                            int32_t* moment_mask, int32_t* boundary_mask, void* stream) {
    if (B == 0) return 0;
    if (!pred_frames || !duration || !bounds_ts || !bound_frames || !moment_mask || !boundary_mask || B < 0 || T < 1)
        return HIREST_E_BADARG;
    hipLaunchKernelGGL(moment_bounds_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pred_frames, duration, n_frames,
                       n_frames_all, T, bounds_ts, bound_frames, moment_mask, boundary_mask);
    return hirest_launch_status();
}

extern "C" int hirest_cascade_boundaries(const int32_t* steps, const int32_t* nsteps, const int32_t* bound_frames,
                                         const double* duration, const int32_t* n_frames, int32_t n_frames_all, int32_t B,
                                         int32_t iters, int32_t* n_bounds, int32_t* bounds, int64_t* step_ts, int32_t* step_frames,
                                         int32_t* step_sample, int32_t* offsets, void* stream) {
    if (!offsets || B < 0 || iters < 0) return HIREST_E_BADARG;
    if (B == 0) return (int)hipMemsetAsync(offsets, 0, sizeof(int32_t), (hipStream_t)stream);
    if ((!steps && iters > 0) || !nsteps || !bound_frames || !duration || !n_bounds || !bounds || !step_ts || !step_frames || !step_sample)
        return HIREST_E_BADARG;
    const int cap = 2 * iters + 4;
    if (cap > CAP_MAX) return HIREST_E_SHAPE;                    // one value per lane
    if ((int64_t)B * (cap - 1) > INT32_MAX) return HIREST_E_SHAPE;
    const dim3 grid((B + 3) / 4), block(256);
    hipLaunchKernelGGL(boundaries_kernel, grid, block, 0, (hipStream_t)stream, steps, nsteps, bound_frames, B, iters, cap, n_bounds,
                       bounds);
    hipLaunchKernelGGL(steps_kernel, grid, block, 0, (hipStream_t)stream, n_bounds, bounds, duration, n_frames, n_frames_all, B, cap,
                       step_ts, step_frames, step_sample, offsets);
    return hirest_launch_status();
}

extern "C" int hirest_cascade_trim_gather(const float* vis, const float* asr, const int32_t* step_frames, const int32_t* step_sample,
                                          int32_t S, int32_t B, int32_t T, int32_t D, int32_t Da, int32_t F, float* out_vis,
                                          float* out_asr, void* stream) {
    if (S == 0) return 0;
    if (!vis || !step_frames || !step_sample || !out_vis || S < 0 || B < 1 || T < 1 || D < 4 || F < 1) return HIREST_E_BADARG;
    if (asr && (!out_asr || Da < 4)) return HIREST_E_BADARG;
    if (D % 4 || (asr && Da % 4)) return HIREST_E_SHAPE;         // whole 16-byte vectors per lane
    if (!aligned16(vis) || !aligned16(out_vis) || (asr && (!aligned16(asr) || !aligned16(out_asr)))) return HIREST_E_BADARG;
    const int64_t rows = (int64_t)S * F;
    if ((rows + 3) / 4 > INT32_MAX) return HIREST_E_SHAPE;
    hipLaunchKernelGGL(trim_gather_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, vis, asr, step_frames,
                       step_sample, rows, B, T, D, Da, F, out_vis, out_asr);
    return hirest_launch_status();
}
