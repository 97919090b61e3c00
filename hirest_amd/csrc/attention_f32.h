// The body of the exact-fp32 flash attention (attention_f32_kernel in joint.hip, whose comments describe the layout), shared with the
// ragged forms of whisper_prefill.hip: one block's NW waves of 32 queries each against T keys of one (sequence, head).  A kernel
// resolves where its block's queries, keys, values and output rows are and calls this; everything a query's bits depend on is here,
// so a query has the same bits in every kernel built around it, whatever NW and whatever else the launch holds.
#pragma once
#include "common.h"

namespace {

// (shared by the attention kernels, the fused multiply-adds written out so that no kernel contracts differently from the
// other: the scale and the additive masks in one rounding, as this kernel has always computed them)
__device__ __forceinline__ float attn_score(float st, float scale, float addc, bool valid) {
    const float sv = __builtin_fmaf(st, scale, addc);
    return valid ? sv : -3.0e38f;
}
__device__ __forceinline__ float attn_lsum(float lrun, float alpha, float psum) { return __builtin_fmaf(lrun, alpha, psum); }

// qbase / kbase / vbase: the head's first float of the sequence's query row 0 / key row 0 / value row 0 (row strides ldq, ldkv, ldkv);
// query q's output goes to out + (orow0 + q) * ldo + ocol.  Tq queries, T keys; qb: which block of 32 NW queries this is (qb * 32 NW
// < Tq).  Query q adds causal_penalty to the scores of keys > q.
template <int DHP, int NW>
__device__ __forceinline__ void attention_f32_block(const float* __restrict__ qbase, int64_t ldq, const float* __restrict__ kbase,
                                                    const float* __restrict__ vbase, int64_t ldkv, float* __restrict__ out, int64_t orow0, int ldo,
                                                    int ocol, int Tq, int T, int qb, int dh, float scale, float add_const, float causal_penalty) {
    constexpr int ALD = DHP + 1, NO = DHP / 32;
    __shared__ float Ks[32 * ALD];
    __shared__ float Vs[32 * ALD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    constexpr int QB = 32 * NW, NT = 64 * NW;                // queries per block, threads per block
    const int q = qb * QB + wave * 32 + l31;
    const bool qvalid = q < Tq;
    // Q^T fragments: B operand [k = d][j = query]: lane holds Q[q][2s + half] for s = 0..DHP/2-1
    // (every load unconditional on a clamped index, the zero chosen afterwards: a guarded load is a memory round trip of its own)
    float qf[DHP / 2];
    const float* qrow = qbase + (int64_t)(qvalid ? q : Tq - 1) * ldq;
#pragma unroll
    for (int s = 0; s < DHP / 2; ++s) {
        const int d = 2 * s + half;
        const float v = qrow[d < dh ? d : dh - 1];
        qf[s] = (qvalid && d < dh) ? v : 0.f;
    }
    f32x16 o[NO];    // O^T rows d = 32 j .. 32 j + 31, column = query
#pragma unroll
    for (int j = 0; j < NO; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[j][e] = 0.f;
    float mrun = -3.0e38f, lrun = 0.f;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // K / V tile staging through registers, one tile ahead (the next tile's rows travel while this one is multiplied: a synchronous
    // load per 32-key tile was a memory round trip in front of every tile, 10 of them at T = 300)
    constexpr int NLD = (32 * (DHP / 4) + NT - 1) / NT;       // float4 per thread and operand: 2 (dh 64) or 3 (96) with four waves
    f32x4 kreg[NLD], vreg[NLD];
    auto fetch_kv = [&](int k0) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            int i = tid + NT * u; i = i < 32 * (DHP / 4) ? i : 32 * (DHP / 4) - 1;
            const int kr = i / (DHP / 4), c = (i - kr * (DHP / 4)) * 4;
            const int key = k0 + kr < T ? k0 + kr : T - 1;
            const int cc = c < dh ? c : dh - 4;                  // (dh % 4 == 0: a 4-vector is inside or outside the head as a whole)
            kreg[u] = *reinterpret_cast<const f32x4*>(kbase + (int64_t)key * ldkv + cc);
            vreg[u] = *reinterpret_cast<const f32x4*>(vbase + (int64_t)key * ldkv + cc);
        }
    };
    fetch_kv(0);
    for (int k0 = 0; k0 < T; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + NT * u;
            if (i < 32 * (DHP / 4)) {
                const int kr = i / (DHP / 4), c = (i - kr * (DHP / 4)) * 4;
                const f32x4 kv = c >= dh ? zero4 : kreg[u], vv = c >= dh ? zero4 : vreg[u];
#pragma unroll
                for (int e = 0; e < 4; ++e) { Ks[kr * ALD + c + e] = kv[e]; Vs[kr * ALD + c + e] = vv[e]; }
            }
        }
        __syncthreads();
        if (k0 + 32 < T) fetch_kv(k0 + 32);
        f32x16 st;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[e] = 0.f;
        // (operand reads in groups of eight, fenced: left to itself the scheduler hoists all DHP / 2 LDS reads of the chain — and the
        //  48 of the P V loop below — in front of the first MFMA, 40-odd live registers that cost the kernel a wave per SIMD)
#pragma unroll
        for (int g8 = 0; g8 < DHP / 2; g8 += 8) {
            float kf[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) kf[i] = Ks[l31 * ALD + 2 * (g8 + i) + half];   // A operand: K[key = l31][d = 2s + half]
#pragma unroll
            for (int i = 0; i < 8; ++i) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[i], qf[g8 + i], st, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        float tmax = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const float sv = attn_score(st[r], scale, key > q ? add_const + causal_penalty : add_const, key < T);
            st[r] = sv;
            tmax = fmaxf(tmax, sv);
        }
        { float pa = tmax, pb = tmax; lane_swap32(pa, pb); tmax = fmaxf(pa, pb); }   // the other half-wave's keys (common.h: wave_max_x)
        const float mnew = fmaxf(mrun, tmax);
        const float alpha = __expf(mrun - mnew);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float pz = __expf(st[r] - mnew); st[r] = pz; psum += pz; }
        { float pa = psum, pb = psum; lane_swap32(pa, pb); psum = pa + pb; }
        lrun = attn_lsum(lrun, alpha, psum);
        mrun = mnew;
#pragma unroll
        for (int j = 0; j < NO; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[j][e] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {   // k-step r: keys kap(r,0) | kap(r,1); A operand V^T[d = l31 (+32 j)][key]
            const int kr = (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
            for (int j = 0; j < NO; ++j)
                o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[kr * ALD + 32 * j + l31], st[r], o[j], 0, 0, 0);
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (!qvalid) return;
    const float inv = 1.0f / lrun;
    float* orow = out + (orow0 + q) * ldo + ocol;
#pragma unroll
    for (int j = 0; j < NO; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // O^T rows (reg&3) + 8*(reg>>2) + 4*half = d
            const int d = 32 * j + 8 * g + 4 * half;
            if (d < dh)
                *reinterpret_cast<f32x4*>(orow + d) = f32x4{o[j][4 * g] * inv, o[j][4 * g + 1] * inv, o[j][4 * g + 2] * inv, o[j][4 * g + 3] * inv};
        }
}

}  // namespace
