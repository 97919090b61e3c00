// Loader batches of the joint model from device-resident features: MomentDataset.__getitem__ + collate_fn
// (hirest_dataset.py:323-531) for a whole batch in one launch.  Every feature file of the corpus was uploaded once
// (hirest_amd/dataset.py: DeviceFeatureStore); a batch is B example numbers, and everything below is index arithmetic on
// integer tables plus row copies.  One wave per output row (b, t): it finds its source rows, copies them 16 bytes per lane and
// writes the row's three mask values; B more waves gather the per-example table rows (targets, token ids, text features).
// No LDS, no atomics, no scratch.  Compiled with -ffp-contract=off: the subsample index is numpy's linspace in double.
#include "common.h"

namespace {

// one row of `D` floats; src == nullptr writes zeros.  vec: D % 4 == 0 and both arrays 16-byte aligned
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int D, bool vec, int lane) {
    if (vec) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
        f32x4* d4 = reinterpret_cast<f32x4*>(dst);
        for (int i = lane; i < D / 4; i += 64) d4[i] = src ? s4[i] : zero;
    } else {
        for (int i = lane; i < D; i += 64) dst[i] = src ? src[i] : 0.f;
    }
}

__global__ void __launch_bounds__(256) assemble_kernel(const hirest_batch_args a, int64_t rows, bool vec, bool vec_asr) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows + a.B) return;                                 // wave-uniform; no workgroup barrier below
    const int b = r < rows ? (int)(r / a.T) : (int)(r - rows);
    const int e = a.index[b];
    const bool ok = e >= 0 && e < a.n_examples;
    if (r >= rows) {                                             // the table rows of example e
        for (int g = 0; g < a.n_gather; ++g) {
            const hirest_batch_gather& it = a.gather[g];
            const int64_t row = ok ? (it.row_of_example ? it.row_of_example[e] : e) : 0;
            const uint32_t* s = static_cast<const uint32_t*>(it.src) + row * it.words;
            uint32_t* d = static_cast<uint32_t*>(it.dst) + (int64_t)b * it.words;
            for (int i = lane; i < it.words; i += 64) d[i] = ok ? s[i] : 0u;
        }
        return;
    }
    const int t = (int)(r - (int64_t)b * a.T);
    const int F = a.n_model_frames;
    int v = 0, L = 0;
    int64_t f0 = 0, n = 0;
    if (ok) {
        v = a.ex_video[e];
        L = a.ex_len[e];
        f0 = a.frame_off[v];
        n = a.frame_off[v + 1] - f0;
    }
    // ---- frame row: hirest_dataset.py:333-356, collate :421-442
    int64_t src = -1;
    if (ok && n > 0) {
        if (F <= 0) src = t;                                                         // as stored; zero rows from n on
        else if (t >= F) src = -1;
        else if (n > F) {
            // np.linspace(0, n - 1, F).astype(int): arange(F) * step in double, the last element overwritten by n - 1
            if (F == 1) src = 0;
            else if (t == F - 1) src = n - 1;
            else src = (int64_t)((double)t * ((double)(n - 1) / (double)(F - 1)));
        } else {
            src = ((int64_t)(t + 1) * n + F - 1) / F - 1;                            // bucket rule: row j fills slots [jF // n, (j + 1)F // n)
        }
        if (src < 0 || src >= n) src = -1;
    }
    copy_row(src >= 0 ? a.frames + (f0 + src) * a.D : nullptr, a.vis + r * a.D, a.D, vec, lane);
    // ---- ASR row: hirest_dataset.py:369-380 on the fitted axis; the later subtitle wins
    if (a.asr_rows) {
        const int64_t fitted = F > 0 ? F : n;
        int best = -1;
        int64_t s0 = 0;
        if (ok && t < fitted) {
            s0 = a.sub_off[v];
            const int ns = (int)(a.sub_off[v + 1] - s0);
            for (int i = lane; i < ns; i += 64) {
                const int st = a.sub_span[2 * (s0 + i)], en = a.sub_span[2 * (s0 + i) + 1];
                if (st <= t && t < en) best = i;                                     // i grows: the lane keeps its last match
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(best, o, 64); best = other > best ? other : best; }
        }
        copy_row(best >= 0 ? a.asr_rows + (s0 + best) * a.Da : nullptr, a.asr + r * a.Da, a.Da, vec_asr, lane);
    }
    // ---- masks: collate :445-491 (zero padding past the example's own length)
    const bool in_len = ok && t < L;
    bool prev = false;
    if (a.prev_boundary_mask && in_len) {
        const int b0 = a.bound_off[e], b1 = a.bound_off[e + 1];
        bool hit = false;
        for (int i = b0 + lane; i < b1; i += 64) hit |= a.bound_val[i] == t;
        prev = __ballot(hit) != 0ull;
    }
    if (lane == 0) {
        bool mm = false;
        if (in_len) {
            const int lo = a.ex_range[3 * e], hi = a.ex_range[3 * e + 1], one = a.ex_range[3 * e + 2];
            mm = (t >= lo && t < hi) || t == one;
        }
        a.vis_mask[r] = in_len ? 1 : 0;
        a.moment_mask[r] = mm ? 1 : 0;
        if (a.prev_boundary_mask) a.prev_boundary_mask[r] = prev ? 1 : 0;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int hirest_batch_assemble(const hirest_batch_args* a, void* stream) {
    if (!a || a->struct_size != sizeof(hirest_batch_args)) return HIREST_E_BADARG;
    if (a->B == 0) return 0;
    if (a->B < 0 || a->T < 1 || a->D < 1 || a->n_examples < 1 || a->n_gather < 0 || a->n_gather > HIREST_BATCH_GATHER_MAX)
        return HIREST_E_BADARG;
    if (!a->index || !a->frames || !a->frame_off || !a->ex_video || !a->ex_len || !a->ex_range || !a->vis || !a->vis_mask || !a->moment_mask)
        return HIREST_E_BADARG;
    if (a->asr_rows && (!a->sub_off || !a->sub_span || !a->asr || a->Da < 1)) return HIREST_E_BADARG;
    if (a->prev_boundary_mask && (!a->bound_off || !a->bound_val)) return HIREST_E_BADARG;
    if (a->n_model_frames > 0 && a->T != a->n_model_frames) return HIREST_E_BADARG;
    for (int g = 0; g < a->n_gather; ++g)
        if (!a->gather[g].src || !a->gather[g].dst || a->gather[g].words < 1) return HIREST_E_BADARG;
    const int64_t rows = (int64_t)a->B * a->T;
    const int64_t groups = (rows + a->B + 3) / 4;
    if (groups > INT32_MAX) return HIREST_E_SHAPE;
    const bool vec = a->D % 4 == 0 && aligned16(a->frames) && aligned16(a->vis);
    const bool vec_asr = a->asr_rows && a->Da % 4 == 0 && aligned16(a->asr_rows) && aligned16(a->asr);
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, *a, rows, vec, vec_asr);
    return hirest_launch_status();
}
