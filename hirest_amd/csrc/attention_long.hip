// Multi-head self-attention core for sequences the short kernels (attention.hip, N <= 272) do not hold on chip: a streaming
// ("flash") bf16 MFMA attention for 64-wide heads, 1 <= N <= 4096, no mask.  ViT-L/14@336px has 577 tokens.
//
// One workgroup (4 waves) per (frame, head, 128-query tile); a wave owns two 16-query tiles and keeps their Q fragments, running
// row maximum / sum and the fp32 O^T accumulators in registers.  K and V stream through LDS in 64-key tiles, double-buffered, both
// ROW-MAJOR by LDS-DMA (global_load_lds_dwordx4) as in attention_kernel_v2; V is consumed through ds_read_b64_tr_b16.  Per key tile:
//   S^T = K . Q^T      v_mfma_f32_16x16x32_bf16(a = K rows from LDS, b = Q fragments): the query (lane & 15) sits in the lane and
//                      the keys in (lane >> 4, register), so a K / V fragment read from LDS feeds both query tiles of the wave
//   online softmax     m' = max(m, tile max); alpha = 2^((m - m') c); p = 2^(s c - m' c) in fp32; l = l alpha + sum p; O^T *= alpha
//   O^T += V^T . P^T   P rounded to bf16, the registers of S^T ARE the B operand (k-slots permuted as in attention.hip)
// and at the end O^T / l is stored as bf16.  The tiling depends on N alone, the row sum is kept per lane and reduced once at the end in
// a fixed order, nothing is atomic: a frame's output bits do not depend on B, on its neighbours or on the run.
// Keys past N exist only in the last key tile: their LDS rows are clamped duplicates of row N - 1 of the SAME frame (never the next
// frame's rows) and their scores are masked to -3e38 before the maximum, so their p is exactly 0.
//
// LDS images (128-B rows = 8 chunks of 16 B; 64 rows per tile):
//   K: chunk c of row r sits at position c ^ ((r >> 1) & 7): the S^T fragment reads (16 rows x one chunk per 16-lane group of
//      ds_read_b128) then hit 16 distinct 16-B slots of the 256-B bank row instead of 2 (rows r and r + 2 share banks at this stride)
//   V: the 32-B block (16 head dims) b of row r sits at block position b ^ ((r >> 1) & 3): the transpose reads fetch rows 4g .. 4g + 3 for
//      two values of g per 32-lane half at one block position, 8 rows that would otherwise share 2 slots
#include "common.h"
#include "profile.h"

namespace {

constexpr int LQ = 128;                 // queries per workgroup: 4 waves x 2 tiles x 16
constexpr int LK = 64;                  // keys per tile
constexpr int LRS = 128;                // LDS row stride, bytes (dh = 64 bf16)
constexpr int LTILE = LK * LRS;         // 8 KiB per K or V tile
constexpr int LBUF = 2 * LTILE;         // K | V of one stage
constexpr int LPIECES = LTILE / 1024 / 4;   // 1-KiB DMA pieces per wave and image: 2

struct RowState {
    float m, l;                         // running maximum (raw score units) and this lane's share of the running sum
    f32x4 o[4];                         // O^T: query (lane & 15), head dims dt * 16 + 4 (lane >> 4) + i
};

// One 64-key step of the online softmax for one 16-query tile: s[t][i] is the raw score of key t * 16 + 4 g + i on entry.
__device__ __forceinline__ void softmax_step(f32x4 (&s)[4], RowState& r, bf16x8 (&p)[2], float c) {
    float mx = s[0][0];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[t][i]);
    { float a = mx, b = mx; lane_swap16(a, b); mx = fmaxf(a, b); a = mx; b = mx; lane_swap32(a, b); mx = fmaxf(a, b); }
    const float mn = fmaxf(r.m, mx);
    const float alpha = __builtin_amdgcn_exp2f((r.m - mn) * c);     // exactly 1 while the maximum stands, 0 on the first tile
    r.m = mn;
    const float nmc = -mn * c;
    float sum = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pz = __builtin_amdgcn_exp2f(fmaf(s[2 * h + u][i], c, nmc));
                sum += pz;
                p[h][4 * u + i] = (bf16_t)pz;
            }
    r.l = fmaf(r.l, alpha, sum);
    if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {           // wave-uniform: most tiles after the first few leave every maximum alone
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 4; ++i) r.o[dt][i] *= alpha;
    }
}

__global__ __launch_bounds__(256, 4) void attention_long_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                            int N, int H, float scale_log2e, int nq, int nqt) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * LBUF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.x / nqt, qt = blockIdx.x - bh * nqt;
    const int b = bh / H, h = bh - b * H;
    const int D = H * 64;
    const int64_t ld = 3 * (int64_t)D;
    const bf16_t* base = qkv + (int64_t)b * N * ld + h * 64;
    const int g = lane >> 4, c16 = lane & 15;
    const int nkt = (N + LK - 1) / LK;

    // ---- LDS-DMA: piece i (1 KiB = 8 rows) of an image is issued by wave i & 3; lane -> (row of the tile, chunk position)
    int prow[LPIECES], pk[LPIECES], pv[LPIECES];
#pragma unroll
    for (int j = 0; j < LPIECES; ++j) {
        const int ci = (wave + 4 * j) * 64 + lane, r = ci >> 3, p = ci & 7;
        prow[j] = r;
        pk[j] = D + (p ^ ((r >> 1) & 7)) * 8;                                  // element offsets inside a qkv row
        pv[j] = 2 * D + (((((p >> 1) ^ ((r >> 1) & 3)) << 1) | (p & 1))) * 8;
    }
    auto dma = [&](int kt) {
        char* dst = smem + (kt & 1) * LBUF;
#pragma unroll
        for (int j = 0; j < LPIECES; ++j) {
            const int key = kt * LK + prow[j];
            const bf16_t* src = base + (int64_t)(key < N ? key : N - 1) * ld;  // clamped inside the frame
            glds16(src + pk[j], dst + (wave + 4 * j) * 1024);
            glds16(src + pv[j], dst + LTILE + (wave + 4 * j) * 1024);
        }
    };

    // ---- this wave's queries: tiles q0 and q0 + 16; rows past N repeat row N - 1 (never stored)
    const int q0 = qt * LQ + wave * 32;
    const bool active = q0 < nq;                                                // wave-uniform; idle waves still stage and synchronise
    bf16x8 qa[2], qb[2];
    {
        const int ra = q0 + c16, rb = q0 + 16 + c16;
        const bf16_t* pa = base + (int64_t)(ra < N ? ra : N - 1) * ld;
        const bf16_t* pb = base + (int64_t)(rb < N ? rb : N - 1) * ld;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            qa[kk] = *reinterpret_cast<const bf16x8*>(pa + (kk * 4 + g) * 8);
            qb[kk] = *reinterpret_cast<const bf16x8*>(pb + (kk * 4 + g) * 8);
        }
    }
    RowState ra_, rb_;
    ra_.m = rb_.m = -3.0e38f;
    ra_.l = rb_.l = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ra_.o[dt] = rb_.o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ksw = c16 >> 1;                               // (row >> 1) & 7 of this lane's K rows (tile rows t * 16 + c16)
    const int vsw = 2 * (g & 1) + (c16 >> 3);               // (row >> 1) & 3 of this lane's V rows (4 g + (c16 >> 2) + 16 k)
    const int koff = c16 * LRS;
    const int voff = (4 * g + (c16 >> 2)) * LRS + (c16 & 3) * 8;

    dma(0);
    for (int kt = 0; kt < nkt; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's pieces of tile kt (and, the first time, its Q fragments)
        __builtin_amdgcn_s_barrier();                       // tile kt landed everywhere; tile kt - 1 is read out everywhere
        asm volatile("" ::: "memory");
        if (kt + 1 < nkt) dma(kt + 1);                      // into the stage tile kt - 1 occupied
        if (!active) continue;
        const char* Ks = smem + (kt & 1) * LBUF;
        const char* Vs = Ks + LTILE;
        f32x4 sa[4], sb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, bq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + t * 16 * LRS + koff + (((kk * 4 + g) ^ ksw) * 16));
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qa[kk], a, 0, 0, 0);
                bq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[kk], bq, 0, 0, 0);
            }
            sa[t] = a;
            sb[t] = bq;
        }
        if (kt == nkt - 1) {                                // only the last tile holds keys past N
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool vis = kt * LK + t * 16 + 4 * g + i < N;
                    sa[t][i] = vis ? sa[t][i] : -3.0e38f;
                    sb[t][i] = vis ? sb[t][i] : -3.0e38f;
                }
        }
        bf16x8 pa[2], pb[2];
        softmax_step(sa, ra_, pa, scale_log2e);
        softmax_step(sb, rb_, pb, scale_log2e);
        // ---- O^T += V^T . P^T: V^T fragments by transpose read, the block rows 4g .. 4g + 3 (+ 16) of each 32-key step
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const char* vrow = Vs + voff + s * 32 * LRS + ((dt ^ vsw) * 32);
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(vrow));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(vrow + 16 * LRS));
                const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                ra_.o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa[s], ra_.o[dt], 0, 0, 0);
                rb_.o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[s], rb_.o[dt], 0, 0, 0);
            }
    }
    if (!active) return;

    // ---- normalise and store: the four lanes (g) of a query add their shares of the row sum in one fixed order
    auto finish = [&](RowState& r, int q) {
        float l = r.l;
        { float a = l, bq = l; lane_swap16(a, bq); l = a + bq; a = l; bq = l; lane_swap32(a, bq); l = a + bq; }
        const float inv = 1.0f / l;
        if (q < nq) {                                       // nq <= N: rows from nq on are left alone
            bf16_t* dst = out + ((int64_t)b * N + q) * D + h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                bf16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (bf16_t)(r.o[dt][i] * inv);
                *reinterpret_cast<bf16x4*>(dst + dt * 16) = o;
            }
        }
    };
    finish(ra_, q0 + c16);
    finish(rb_, q0 + 16 + c16);
}

}  // namespace

extern "C" int hirest_attention_bf16_long(const hirest_bf16* qkv, hirest_bf16* out, int32_t B, int32_t N, int32_t H, int32_t dh,
                                          float scale, int32_t q_rows, void* stream) {
    if (!qkv || !out || B <= 0 || H <= 0 || q_rows < 0) return HIREST_E_BADARG;
    if (N < 1 || N > 4096 || dh != 64) return HIREST_E_SHAPE;
    const int nq = (q_rows == 0 || q_rows > N) ? N : q_rows;
    const int nqt = (nq + LQ - 1) / LQ;                     // with q_rows set only the leading query tiles are computed
    const int64_t grid = (int64_t)B * H * nqt;
    if (grid > 0x7fffffff) return HIREST_E_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HirestProfScope prof(HIREST_PROF_ATTENTION, 2, (int64_t)B * H, N, dh, s);   // tag 2: this entry (0 / 1: the short ones' causal flag)
    hipLaunchKernelGGL(attention_long_kernel, dim3((unsigned)grid), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(qkv),
                       reinterpret_cast<bf16_t*>(out), N, H, scale * 1.44269504088896340736f, nq, nqt);
    return hirest_launch_status();
}
