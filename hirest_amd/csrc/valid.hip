// The validation pass of the joint model (hirest_amd/moment_model.py: valid_step): loss AND prediction from one forward.
//
// hirest_moment_valid_f32 — moment retrieval (modeling.py:226-310): from the [2, B T] start / end head logits, the masked arg-max of
//   test_moment_retrieval (fill where vis_mask == 0, first maximum) and the training loss (BCE_start + BCE_end) / 2, each sum over
//   moment_mask divided by max(sum moment_mask, 1) of the whole batch.  ONE block: wave w owns samples w, w + 16, ...; a sample's two
//   indices, two BCE sums and mask count are reduced inside its wave in a fixed lane order (double accumulators), parked in LDS, and
//   thread 0 adds the per-sample partials in sample order.  No atomics: repeated calls give the same bits, and a sample's indices
//   see nothing of the other samples.
//
// hirest_lm_head_ce_f32 — step captioning (modeling.py:519): CrossEntropyLoss(ignore_index = -1) of h W^T + b over the vocabulary
//   without a logit ever reaching memory.  Exact fp32 products on v_mfma_f32_32x32x2_f32.  A block owns 32 rows of h (staged once
//   into LDS, 96.5 KB) and one 512-column slice of the vocabulary; each of its four waves takes 32-column tiles of the slice, streams
//   the tile's W rows HBM -> registers through an 8-deep ring of 64-byte pieces (W is read once per block and shared by nobody inside
//   it, so an LDS round trip would be pure overhead) and keeps, per row, the running maximum, the sum of exponentials (double) and
//   the target's logit.  One partial (max, target logit, sum) per (row, slice); a second small kernel merges a row's slices in index
//   order and forms the mean in row order.  The slice width is a constant and every row's arithmetic is its own, so a row's nll does
//   not depend on how many other rows there are.
#include "common.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------ moment retrieval
constexpr int MV_THREADS = 1024, MV_WAVES = MV_THREADS / 64, MV_MAX_B = 1024;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(MV_THREADS) void moment_valid_kernel(const float* __restrict__ logits, const int32_t* __restrict__ vis_mask,
                                                                  const int32_t* __restrict__ moment_mask,
                                                                  const int32_t* __restrict__ start_target,
                                                                  const int32_t* __restrict__ end_target, int B, int T, float fill,
                                                                  int32_t* __restrict__ pred, float* __restrict__ loss) {
    __shared__ double part[3 * MV_MAX_B];                    // per sample: BCE sum of the start head, of the end head, mask count
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)B * T;
    for (int b = wave; b < B; b += MV_WAVES) {               // (wave-uniform)
        const int64_t o = (int64_t)b * T;
        const int tg[2] = {start_target[b], end_target[b]};
        double cnt = 0.0;
        for (int t = lane; t < T; t += 64) cnt += (double)moment_mask[o + t];
        part[3 * b + 2] = wave_sum_d(cnt);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* lg = logits + h * rows + o;
            float best = -INFINITY; int bi = 0x7fffffff;
            double s = 0.0;
            for (int t = lane; t < T; t += 64) {
                const float x = lg[t];
                const float v = vis_mask[o + t] ? x : fill;
                if (v > best || (v == best && t < bi)) { best = v; bi = t; }
                // max(x, 0) - x y + log(1 + exp(-|x|)): torch's stable form, in double
                const double xd = (double)x, y = t == tg[h] ? 1.0 : 0.0;
                s += (double)moment_mask[o + t] * (fmax(xd, 0.0) - xd * y + log1p(exp(-fabs(xd))));
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const float ov = __shfl_xor(best, d, 64); const int oi = __shfl_xor(bi, d, 64);
                if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            s = wave_sum_d(s);
            if (lane == 0) { pred[2 * b + h] = bi; part[3 * b + h] = s; }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                  // the ordered pass over the samples
        double ss = 0.0, se = 0.0, c = 0.0;
        for (int b = 0; b < B; ++b) { ss += part[3 * b]; se += part[3 * b + 1]; c += part[3 * b + 2]; }
        const double denom = c > 1.0 ? c : 1.0;
        *loss = (float)((ss / denom + se / denom) * 0.5);
    }
}

// ------------------------------------------------------------------------------------------------------------ LM head + CE
constexpr int CE_K = 768, CE_LD = CE_K + 4;                  // LDS row stride: + 16 B, so the 32 rows of a ds_read_b128 spread over the banks
constexpr int CE_ROWS = 32, CE_TILE = 32, CE_SLICE_TILES = 16, CE_SLICE = CE_TILE * CE_SLICE_TILES;
constexpr int CE_RING = 8, CE_KSTEP = 16, CE_STEPS = CE_K / CE_KSTEP;     // a ring piece: 16 k of one W row pair (8 per lane half)
constexpr int CE_LDS = (CE_ROWS * CE_LD + CE_SLICE) * 4 + 4 * CE_ROWS * 16;
constexpr float CE_NEG = -3.0e38f;                           // "no column yet": finite, so that no inf - inf can arise
static_assert(CE_STEPS % CE_RING == 0, "ring slots are compile-time inside the k loop");

struct CePartial { float m, tl; double s; };                 // running maximum, the target's logit (0 where the slice has none), sum exp(x - m)

__device__ __forceinline__ void ce_merge(float& m, double& s, float m2, double s2) {      // (m, s) <- (m, s) then (m2, s2)
    const float M = fmaxf(m, m2);
    s = s * (double)expf(m - M) + s2 * (double)expf(m2 - M);
    m = M;
}

__global__ __launch_bounds__(256) void lm_head_ce_partial_kernel(const float* __restrict__ h, int64_t ldh, const float* __restrict__ W,
                                                                 int64_t ldw, const float* __restrict__ bias,
                                                                 const int32_t* __restrict__ target, int R, int V, int nslice,
                                                                 CePartial* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* hs = reinterpret_cast<float*>(smem);              // [32][772]
    float* bias_lds = hs + CE_ROWS * CE_LD;                  // [512]
    CePartial* wred = reinterpret_cast<CePartial*>(bias_lds + CE_SLICE);      // [4][32]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const int M0 = (int)blockIdx.x * CE_ROWS, slice = (int)blockIdx.y, n0 = slice * CE_SLICE;
    // the block's 32 rows of h (rows past R repeat row R - 1 and are never written back) and the slice's bias
    constexpr int HV = CE_ROWS * (CE_K / 4) / 256, HB = 12;  // 24 float4 per thread, 12 loads in flight at a time
    static_assert(CE_ROWS * (CE_K / 4) % 256 == 0 && HV % HB == 0, "whole batches of loads");
#pragma unroll 1
    for (int i0 = 0; i0 < HV; i0 += HB) {
        f32x4 v[HB];
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const int i = tid + 256 * (i0 + u), r = i / (CE_K / 4), c4 = i - r * (CE_K / 4);
            int gm = M0 + r; gm = gm < R ? gm : R - 1;
            v[u] = *reinterpret_cast<const f32x4*>(h + (int64_t)gm * ldh + 4 * c4);
        }
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const int i = tid + 256 * (i0 + u), r = i / (CE_K / 4), c4 = i - r * (CE_K / 4);
            *reinterpret_cast<f32x4*>(hs + r * CE_LD + 4 * c4) = v[u];
        }
    }
    for (int i = tid; i < CE_SLICE; i += 256) bias_lds[i] = n0 + i < V ? bias[n0 + i] : 0.f;
    __syncthreads();

    int mine = 0;                                            // tiles wave, wave + 4, ... of the slice that start inside the vocabulary
    for (int u = 0; u < CE_SLICE_TILES / 4; ++u) mine += n0 + CE_TILE * (wave + 4 * u) < V ? 1 : 0;
    const int row = M0 + j;
    const int tgt = row < R ? target[row] : -1;
    float m = CE_NEG, tl = 0.f;
    double s = 0.0;
    if (mine > 0) {                                          // (wave-uniform)
        // the W stream of this wave: piece q of tile u = floats 16 q + 8 hf .. + 7 of row n0 + 32 (wave + 4 u) + j (rows past V - 1 repeat it)
        auto wrow = [&](int u) {
            int n = n0 + CE_TILE * (wave + 4 * u) + j; n = n < V ? n : V - 1;
            return W + (int64_t)n * ldw + 8 * hf;
        };
        int pu = 0, pq = 0;
        const float* prow = wrow(0);
        auto fetch = [&](f32x4 (&dst)[2]) {
            const float* p = prow + CE_KSTEP * pq;
            dst[0] = *reinterpret_cast<const f32x4*>(p);
            dst[1] = *reinterpret_cast<const f32x4*>(p + 4);
            if (++pq == CE_STEPS) {
                if (pu + 1 < mine) { pq = 0; ++pu; prow = wrow(pu); }
                else pq = CE_STEPS - 1;                      // past the end of the stream: the last piece again (never used)
            }
        };
        f32x4 ring[CE_RING][2];
#pragma unroll
        for (int d = 0; d < CE_RING; ++d) fetch(ring[d]);
        const float* hl = hs + j * CE_LD + 8 * hf;
#pragma unroll 1
        for (int u = 0; u < mine; ++u) {
            f32x16 acc[4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
#pragma unroll 1
            for (int qo = 0; qo < CE_STEPS; qo += CE_RING) {
#pragma unroll
                for (int d = 0; d < CE_RING; ++d) {
                    const f32x4 w0 = ring[d][0], w1 = ring[d][1];
                    const float* hp = hl + CE_KSTEP * (qo + d);
                    const f32x4 b0 = *reinterpret_cast<const f32x4*>(hp), b1 = *reinterpret_cast<const f32x4*>(hp + 4);
                    // A = W (vocabulary index on the MFMA's rows), B = h (row of h on the lane's column): lane half hf brings k = 16 q + 8 hf + e
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[e], b0[e], acc[e], 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[e], b1[e], acc[e], 0, 0, 0);
                    fetch(ring[d]);
                }
            }
            // the tile's 16 logits of this lane: column j = row of h, register e = vocabulary index (e & 3) + 8 (e >> 2) + 4 hf
            const int tl_idx = wave + 4 * u, v0 = n0 + CE_TILE * tl_idx;
            float x[16], tmax = CE_NEG;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = (e & 3) + 8 * (e >> 2) + 4 * hf;
                x[e] = ((acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e])) + bias_lds[CE_TILE * tl_idx + i];
                if (v0 + i < V) tmax = fmaxf(tmax, x[e]);
                if (v0 + i == tgt) tl = x[e];
            }
            const float mn = fmaxf(m, tmax);
            double add = 0.0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = (e & 3) + 8 * (e >> 2) + 4 * hf;
                if (v0 + i < V) add += (double)expf(x[e] - mn);
            }
            s = s * (double)expf(m - mn) + add;
            m = mn;
        }
    }
    // the two lane halves of a row (half 0 first), then the four waves in wave order
    {
        const float om = __shfl_xor(m, 32, 64), otl = __shfl_xor(tl, 32, 64);
        const double os = __shfl_xor(s, 32, 64);
        float ma = hf ? om : m, mb = hf ? m : om;
        double sa = hf ? os : s, sb = hf ? s : os;
        ce_merge(ma, sa, mb, sb);
        if (hf == 0) wred[wave * CE_ROWS + j] = CePartial{ma, tl + otl, sa};
    }
    __syncthreads();
    if (tid < CE_ROWS && M0 + tid < R) {
        CePartial p = wred[tid];
        for (int w = 1; w < 4; ++w) {
            const CePartial q = wred[w * CE_ROWS + tid];
            ce_merge(p.m, p.s, q.m, q.s);
            p.tl += q.tl;
        }
        part[(int64_t)(M0 + tid) * nslice + slice] = p;
    }
}

// nll[r] = log sum exp - target logit from the row's slices in index order; *loss = mean of the rows with target >= 0, in row order
__global__ __launch_bounds__(256) void lm_head_ce_merge_kernel(const CePartial* __restrict__ part, const int32_t* __restrict__ target, int R,
                                                               int nslice, int n_valid, float* __restrict__ nll, float* __restrict__ loss) {
    for (int r = threadIdx.x; r < R; r += 256) {
        float out = 0.f;
        if (target[r] >= 0) {
            const CePartial* p = part + (int64_t)r * nslice;
            float M = CE_NEG;
            for (int i = 0; i < nslice; ++i) M = fmaxf(M, p[i].m);
            double S = 0.0, tl = 0.0;
            for (int i = 0; i < nslice; ++i) { S += p[i].s * exp((double)p[i].m - (double)M); tl += (double)p[i].tl; }
            out = (float)(((double)M + log(S)) - tl);
        }
        nll[r] = out;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
#pragma unroll 8
        for (int r = 0; r < R; ++r) acc += (double)nll[r];
        *loss = (float)(acc / (double)(n_valid > 0 ? n_valid : 1));
    }
}

}  // namespace

extern "C" int hirest_moment_valid_f32(const float* logits, const int32_t* vis_mask, const int32_t* moment_mask, const int32_t* start_target,
                                       const int32_t* end_target, int32_t B, int32_t T, float fill, int32_t* pred, float* loss, void* stream) {
    if (!logits || !vis_mask || !moment_mask || !start_target || !end_target || !pred || !loss || B <= 0 || T <= 0 || B > MV_MAX_B)
        return HIREST_E_BADARG;
    hipLaunchKernelGGL(moment_valid_kernel, dim3(1), dim3(MV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, vis_mask,
                       moment_mask, start_target, end_target, B, T, fill, pred, loss);
    return hirest_launch_status();
}

extern "C" size_t hirest_lm_head_ce_workspace_bytes(int32_t R, int32_t V) {
    if (R <= 0 || V <= 0) return 0;
    return (size_t)R * (size_t)((V + CE_SLICE - 1) / CE_SLICE) * sizeof(CePartial);
}

extern "C" int hirest_lm_head_ce_f32(const float* h, int64_t ldh, const float* W, int64_t ldw, const float* bias, const int32_t* target,
                                     int32_t R, int32_t V, int32_t K, int32_t n_valid, float* nll, float* loss, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!h || !W || !bias || !target || !nll || !loss || !workspace || R <= 0 || V <= 0 || K <= 0 || n_valid < 0) return HIREST_E_BADARG;
    if (ldh < K || ldw < K || ldh % 4 || ldw % 4) return HIREST_E_BADARG;
    if (K != CE_K) return HIREST_E_SHAPE;
    if (workspace_bytes < hirest_lm_head_ce_workspace_bytes(R, V)) return HIREST_E_WORKSPACE;
    static HirestDevCfg cfg;
    if (int e = hirest_configure(lm_head_ce_partial_kernel, CE_LDS, cfg)) return e;
    const int nslice = (V + CE_SLICE - 1) / CE_SLICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    CePartial* part = reinterpret_cast<CePartial*>(workspace);
    hipLaunchKernelGGL(lm_head_ce_partial_kernel, dim3((R + CE_ROWS - 1) / CE_ROWS, nslice), dim3(256), CE_LDS, s, h, ldh, W, ldw, bias,
                       target, R, V, nslice, part);
    if (int e = hirest_launch_status()) return e;
    hipLaunchKernelGGL(lm_head_ce_merge_kernel, dim3(1), dim3(256), 0, s, part, target, R, nslice, n_valid, nll, loss);
    return hirest_launch_status();
}
