// BERTScore's greedy matching (evaluate.py:294-297 calls bert_score.score): per (candidate, reference) pair the cosine of every
// candidate token state with every reference token state, the row and column maxima, and their weighted means P, R and F.
//
// One block of four waves per pair.  Phase 1: the L2 norm of each of the pair's rows (one wave per row, lanes stride the
// float4s, xor butterfly).  Phase 2: the cosine matrix in 32 x 32 tiles on v_mfma_f32_32x32x2_f32 (exact fp32): wave w owns the
// candidate row tiles w, w + 4, ... and walks every reference tile for each.  A lane reads one float4 of its candidate row and one of
// its reference row straight from global memory, divides each by the row's norm and feeds four MFMAs; the tile lives only in the 16
// accumulator registers.  Row maxima stay in registers across the reference tiles, column maxima go to the wave's own LDS row.
// Lanes past a sentence's end feed zeros and are set to -inf before any max.  Phase 3: one lane adds w_i * max_i in token order.
// Nothing depends on n_pairs, on the pair's place in the batch or on another pair's rows.
#include "common.h"

#include <math.h>

namespace {

constexpr int BS_MAXLEN = HIREST_BERTSCORE_MAX_TOKENS;
constexpr int BS_WAVES = 4;

// sum of squares of one row by one wave; every lane returns the same bits
__device__ __forceinline__ float row_norm(const float* __restrict__ row, int D, int lane) {
    float s = 0.f;
    for (int c = lane; c < (D >> 2); c += 64) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + 4 * c);
        s = fmaf(x[0], x[0], s); s = fmaf(x[1], x[1], s); s = fmaf(x[2], x[2], s); s = fmaf(x[3], x[3], s);
    }
    return sqrtf(wave_sum(s));
}

// the maximum over the 32 lanes that share lane >> 5 (the columns of one accumulator row)
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(64 * BS_WAVES) void bertscore_greedy_kernel(
        const float* __restrict__ states, int64_t ld, int D, const int32_t* __restrict__ seq_off, int n_seq,
        const float* __restrict__ tok_weight, const int32_t* __restrict__ cand_seq, const int32_t* __restrict__ ref_seq,
        float* __restrict__ out) {
    __shared__ float norm_c[BS_MAXLEN], norm_r[BS_MAXLEN];     // L2 norms of the candidate / reference rows
    __shared__ float max_c[BS_MAXLEN];                         // wp: best reference cosine of each candidate token
    __shared__ float max_r[BS_WAVES][BS_MAXLEN];               // wr per wave (each wave sees its own candidate row tiles)
    __shared__ float pr[2];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* o = out + (int64_t)pair * 3;
    const int cs = cand_seq[pair], rs = ref_seq[pair];
    const float nan = __builtin_nanf("");
    if (cs < 0 || cs >= n_seq || rs < 0 || rs >= n_seq) {       // block-uniform: nothing of the states is read
        if (tid < 3) o[tid] = nan;
        return;
    }
    const int c0 = seq_off[cs], r0 = seq_off[rs];
    const int Lc = seq_off[cs + 1] - c0, Lr = seq_off[rs + 1] - r0;
    if (Lc < 1 || Lr < 1 || Lc > BS_MAXLEN || Lr > BS_MAXLEN) {
        if (tid < 3) o[tid] = nan;
        return;
    }
    const float* C = states + (int64_t)c0 * ld;
    const float* R = states + (int64_t)r0 * ld;

    for (int i = wave; i < Lc; i += BS_WAVES) {
        const float n = row_norm(C + (int64_t)i * ld, D, lane);
        if (lane == 0) norm_c[i] = n;
    }
    for (int j = wave; j < Lr; j += BS_WAVES) {
        const float n = row_norm(R + (int64_t)j * ld, D, lane);
        if (lane == 0) norm_r[j] = n;
    }
    for (int j = tid; j < Lr; j += 64 * BS_WAVES)
#pragma unroll
        for (int w = 0; w < BS_WAVES; ++w) max_r[w][j] = -INFINITY;
    __syncthreads();

    const int l31 = lane & 31, half = lane >> 5;
    const int kcol = 4 * half;                                  // this lane's float4 inside a step of 8 columns
    for (int ti = wave; ti * 32 < Lc; ti += BS_WAVES) {
        const int i = ti * 32 + l31;                            // operand row of this lane
        const bool iv = i < Lc;
        const float* arow = C + (int64_t)(iv ? i : 0) * ld;
        const float an = iv ? norm_c[i] : 1.f;
        f32x16 rmax;
#pragma unroll
        for (int r = 0; r < 16; ++r) rmax[r] = -INFINITY;
        for (int tj = 0; tj * 32 < Lr; ++tj) {
            const int j = tj * 32 + l31;
            const bool jv = j < Lr;
            const float* brow = R + (int64_t)(jv ? j : 0) * ld;
            const float bn = jv ? norm_r[j] : 1.f;
            f32x16 acc = {};
            for (int k0 = 0; k0 < D; k0 += 8) {
                const int k = k0 + kcol;
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
                if (k < D) {                                    // D % 4 == 0: a float4 is inside the row or wholly past it
                    if (iv) a = *reinterpret_cast<const f32x4*>(arow + k);
                    if (jv) b = *reinterpret_cast<const f32x4*>(brow + k);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] /= an; b[e] /= bn;                     // the unit vectors of the definition, then their exact fp32 dot
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
                }
            }
            // acc[r] = sim[ti*32 + (r & 3) + 8 (r >> 2) + 4 half][tj*32 + l31]
            float cmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v = (jv && row < Lc) ? acc[r] : -INFINITY;
                rmax[r] = fmaxf(rmax[r], v);
                cmax = fmaxf(cmax, v);
            }
            cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
            if (half == 0 && jv) max_r[wave][j] = fmaxf(max_r[wave][j], cmax);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float m = half_max(rmax[r]);
            const int row = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (l31 == 0 && row < Lc) max_c[row] = m;
        }
    }
    __syncthreads();

    // weighted means, added in token order by one lane each: P by wave 0, R by wave 1
    if (tid == 0) {
        float num = 0.f, den = 0.f;
        for (int i = 0; i < Lc; ++i) {
            const float w = tok_weight[c0 + i];
            num = fmaf(w, max_c[i], num);
            den += w;
        }
        pr[0] = den == 0.f ? 0.f : num / den;
    }
    if (tid == 64) {
        float num = 0.f, den = 0.f;
        for (int j = 0; j < Lr; ++j) {
            const float w = tok_weight[r0 + j];
            float m = max_r[0][j];
#pragma unroll
            for (int w2 = 1; w2 < BS_WAVES; ++w2) m = fmaxf(m, max_r[w2][j]);
            num = fmaf(w, m, num);
            den += w;
        }
        pr[1] = den == 0.f ? 0.f : num / den;
    }
    __syncthreads();
    if (tid == 0) {
        const float P = pr[0], Rr = pr[1];
        float F = 2.f * P * Rr / (P + Rr);
        if (F != F) F = 0.f;
        o[0] = P; o[1] = Rr; o[2] = F;
    }
}

}  // namespace

extern "C" int hirest_bertscore_greedy(const float* states, int64_t ld, int32_t D, const int32_t* seq_off, int32_t n_seq,
                                       const float* tok_weight, const int32_t* cand_seq, const int32_t* ref_seq, int32_t n_pairs,
                                       float* out, void* stream) {
    if (!states || !seq_off || !tok_weight || !cand_seq || !ref_seq || !out) return HIREST_E_BADARG;
    if (D < 4 || D % 4 != 0 || ld < D || ld % 4 != 0 || n_seq < 1 || n_pairs < 0) return HIREST_E_BADARG;
    if (n_pairs == 0) return 0;
    hipLaunchKernelGGL(bertscore_greedy_kernel, dim3(n_pairs), dim3(64 * BS_WAVES), 0, reinterpret_cast<hipStream_t>(stream), states, ld,
                       (int)D, seq_off, (int)n_seq, tok_weight, cand_seq, ref_seq, out);
    return hirest_launch_status();
}
