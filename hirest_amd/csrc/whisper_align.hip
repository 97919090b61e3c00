// Word-level timestamps for Whisper on gfx950: what whisper/timing.py does on the cross-attention weights of a
// teacher-forced pass.  Two entry points: the alignment matrix of one window (scores of the selected heads, softmax over the first
// n_keys keys, per-column normalisation over the tokens, median filter along the keys, mean over the heads) and dynamic time warping
// over it.  Every reduction has a fixed order (the house rule of whisper_dec.hip): a window's matrix has the same bits on every run
// and whatever else ran in the workspace before; a DTW cell is one fp32 addition of determined operands.
#include "common.h"
#include <math.h>

namespace {

__device__ __forceinline__ float bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Step 1a, scores.  One launch per layer that has selected heads; a block of four waves per (selected head, chunk of 64 keys) stages
// the chunk's key rows for its head in LDS once, as cross_partial_kernel does (rows padded to 68 floats), and serves every token from
// it: wave v takes tokens v, v + 4, ...; lane = key; q . k over d = 0 .. 63 in order.  Keys past n_keys are never read (the staging
// re-reads key n_keys - 1 and the store is masked), so nothing depends on what the window holds behind them.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int ACH = 64, AKLD = 68, AHEADS = 64;

struct AlignLayer {
    const float* q; int64_t ldq;          // this layer's cross-attention query rows [T, D]
    const float* kv; int64_t ldkv;        // the window's key | value rows [Tk, 2 D]
    int n_heads, T, n_keys, nchunk;
    float scale;
    float* w;                             // [n_sel, T, n_keys]
    int16_t head[AHEADS], sel[AHEADS];    // the layer's selected heads and their index s
};

__global__ __launch_bounds__(256) void align_scores_kernel(AlignLayer p) {
    __shared__ __attribute__((aligned(16))) float Ks[ACH * AKLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x % p.nchunk, e = blockIdx.x / p.nchunk;
    const int h = p.head[e], s = p.sel[e], k0 = c * ACH;
    const float* base = p.kv + h * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, key = k0 + (idx >> 4), kk = key < p.n_keys ? key : p.n_keys - 1;
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(base + (int64_t)kk * p.ldkv + 4 * (idx & 15));
        *reinterpret_cast<f32x4*>(Ks + (idx >> 4) * AKLD + 4 * (idx & 15)) = k4;
    }
    __syncthreads();
    float* wrow = p.w + (int64_t)s * p.T * p.n_keys + k0 + lane;
    for (int t = wave; t < p.T; t += 4) {                         // (wave-uniform)
        const float qv = p.q[(int64_t)t * p.ldq + h * 64 + lane];
        float st = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < 16; ++c4) {
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(Ks + lane * AKLD + 4 * c4);
#pragma unroll
            for (int d = 0; d < 4; ++d) st = __builtin_fmaf(k4[d], bcast(qv, 4 * c4 + d), st);
        }
        if (k0 + lane < p.n_keys) wrow[(int64_t)t * p.n_keys] = st * p.scale;
    }
}

// Step 1b, softmax in place.  One wave per (s, t) row: a lane's keys lane, lane + 64, ... in ascending order, then the xor-shuffle
// tree; the exponentials are stored by the second pass and divided by their sum in the third.
__global__ __launch_bounds__(256) void align_softmax_kernel(float* w, int64_t rows, int n_keys) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                      // (wave-uniform; no barrier below)
    float* x = w + row * n_keys;
    float m = -3.0e38f;
    for (int j = lane; j < n_keys; j += 64) m = fmaxf(m, x[j]);
    m = wave_max(m);
    float l = 0.f;
    for (int j = lane; j < n_keys; j += 64) {
        const float e = expf(x[j] - m);
        x[j] = e;
        l += e;
    }
    l = wave_sum(l);
    for (int j = lane; j < n_keys; j += 64) x[j] = x[j] / l;
}

// Step 2.  One thread per (s, key): mean and population standard deviation over the T tokens in ascending order (two passes), then
// (w - mean) / std in place.  Neighbouring threads read neighbouring keys.
__global__ __launch_bounds__(256) void align_normalize_kernel(float* w, int n_sel, int T, int n_keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n_sel * n_keys) return;
    const int s = (int)(i / n_keys), j = (int)(i - (int64_t)s * n_keys);
    float* x = w + (int64_t)s * T * n_keys + j;
    float sum = 0.f;
    for (int t = 0; t < T; ++t) sum += x[(int64_t)t * n_keys];
    const float mean = sum / (float)T;
    float q = 0.f;
    for (int t = 0; t < T; ++t) { const float d = x[(int64_t)t * n_keys] - mean; q = __builtin_fmaf(d, d, q); }
    const float sd = sqrtf(q / (float)T);
    for (int t = 0; t < T; ++t) x[(int64_t)t * n_keys] = (x[(int64_t)t * n_keys] - mean) / sd;
}

// Steps 3 and 4.  A block per (output row, tile of 256 keys) walks s in ascending order: the tile of row (s, row0 + r) with its
// reflected margins goes to LDS, every thread selects the median of its window — the element with at most width / 2 smaller ones and
// more than width / 2 smaller-or-equal ones, counted, so the value is exact and no array is indexed in registers — and adds it to
// its sum; out = sum / n_sel.  width 1, or a row of at most width / 2 keys (Whisper's early return), passes the value through.
constexpr int MTILE = 256, MWIDTH_MAX = 31;

__global__ __launch_bounds__(MTILE) void align_median_mean_kernel(const float* __restrict__ w, int n_sel, int T, int n_keys, int width,
                                                                  int row0, float* __restrict__ out, int n_tiles) {
    __shared__ float S[MTILE + MWIDTH_MAX - 1];
    const int tid = threadIdx.x, r = blockIdx.x / n_tiles, j0 = (blockIdx.x - r * n_tiles) * MTILE, j = j0 + tid;
    const int p = n_keys <= width / 2 ? 0 : width / 2, span = 2 * p + 1;
    float acc = 0.f;
    for (int s = 0; s < n_sel; ++s) {
        const float* x = w + ((int64_t)s * T + row0 + r) * n_keys;
        for (int i = tid; i < MTILE + 2 * p; i += MTILE) {
            int jj = j0 - p + i;
            if (jj < 0) jj = -jj;
            if (jj >= n_keys) jj = 2 * (n_keys - 1) - jj;
            jj = jj < 0 ? 0 : (jj >= n_keys ? n_keys - 1 : jj);   // (behind the row's end in its last tile: not used)
            S[i] = x[jj];
        }
        __syncthreads();
        float med = S[tid + p];
        for (int a = 0; a < span; ++a) {
            const float va = S[tid + a];
            int less = 0, eq = 0;
            for (int b = 0; b < span; ++b) {
                const float vb = S[tid + b];
                less += vb < va;
                eq += vb == va;
            }
            if (less <= p && p < less + eq) med = va;
        }
        acc += med;
        __syncthreads();
    }
    if (j < n_keys) out[(int64_t)r * n_keys + j] = acc / (float)n_sel;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Dynamic time warping.  One workgroup per problem, thread r owns row r and walks the anti-diagonals: on diagonal d it is at column
// d - r.  Of its three predecessors one is its own last value; the other two are row r - 1's last value and the one before, so ONE
// value moves per diagonal: by a cross-lane shift inside a wave, through a double-buffered LDS slot from lane 63 to the next wave's
// lane 0, with one barrier per diagonal.  A row's x values are fetched a round of four diagonals ahead.  The trace goes to the
// workspace as 2-bit codes, 16 columns to a word, written by the row's thread as a word fills.  After the last diagonal lane 0
// walks back from (N, M) — it re-reads a trace word only when the row or the word changes — writing the reversed list into the
// workspace, and the whole block copies it out in order.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int DTW_BATCH = 16;

struct DtwItem {
    const float* x; int64_t ldx;
    float* cost; int64_t ldc;
    int32_t* path; int32_t* path_len;
    uint32_t* trace; int32_t* rev;
    int N, M, negate, pad;
};
struct DtwBatch { DtwItem item[DTW_BATCH]; };

__global__ __launch_bounds__(256) void dtw_kernel(DtwBatch batch) {
    __shared__ float edge[2][4];
    __shared__ int n_path;
    const DtwItem& p = batch.item[blockIdx.x];
    const int r = threadIdx.x, lane = r & 63, wave = r >> 6, N = p.N, M = p.M, words = (M + 15) >> 4;
    const float INF = __builtin_inff();
    if (r < 8) edge[r >> 2][r & 3] = INF;
    __syncthreads();
    const bool mine = r < N;
    const float* xr = p.x + (int64_t)(mine ? r : 0) * p.ldx;
    float left = INF, upleft = r == 0 ? 0.f : INF, cur = INF;
    uint32_t packed = 0;
    // (unconditional, from a clamped column — of row 0 for the threads past N: a round issues exactly four loads, so the wait for a
    //  round's values can leave the next round's in flight)
    auto fetch = [&](int c) { return xr[c < 0 ? 0 : (c >= M ? M - 1 : c)]; };
    auto step = [&](int d, float x) {                                             // anti-diagonal d; x = x[r, d - r] where that cell exists
        float up = __shfl_up(cur, 1, 64);
        if (lane == 0) up = wave > 0 ? edge[(d + 1) & 1][wave - 1] : INF;         // what lane 63 of the wave before left on diagonal d - 1
        const int c = d - r;
        if (mine && c >= 0 && c < M) {
            const float xv = p.negate ? -x : x;
            const float c0 = upleft, c1 = up, c2 = left;
            float best; uint32_t code;
            if (c0 < c1 && c0 < c2) { best = c0; code = 0; }
            else if (c1 < c0 && c1 < c2) { best = c1; code = 1; }
            else { best = c2; code = 2; }
            cur = xv + best;
            left = cur;
            upleft = up;
            if (p.cost) p.cost[(int64_t)r * p.ldc + c] = cur;
            packed |= code << (2 * (c & 15));
            if ((c & 15) == 15 || c == M - 1) {
                p.trace[(int64_t)r * words + (c >> 4)] = packed;
                packed = 0;
            }
        }
        if (lane == 63) edge[d & 1][wave] = cur;
        __syncthreads();
    };
    // Four diagonals per round, the same four for every lane, so that the wave's load counter is waited on once a round and for loads
    // issued a round before: the x values of diagonals d0 + 4 .. d0 + 7 are fetched while d0 .. d0 + 3 run.  (Diagonals past the last
    // one, up to three, find no cell.)
    float b0 = fetch(0 - r), b1 = fetch(1 - r), b2 = fetch(2 - r), b3 = fetch(3 - r);
    for (int d0 = 0; d0 < N + M - 1; d0 += 4) {
        const float a0 = b0, a1 = b1, a2 = b2, a3 = b3;
        b0 = fetch(d0 + 4 - r); b1 = fetch(d0 + 5 - r); b2 = fetch(d0 + 6 - r); b3 = fetch(d0 + 7 - r);
        step(d0, a0); step(d0 + 1, a1); step(d0 + 2, a2); step(d0 + 3, a3);
    }
    __threadfence_block();
    __syncthreads();
    if (r == 0) {
        int i = N, j = M, n = 0, wi = -1, wj = -1;
        uint32_t word = 0;
        while (i > 0 || j > 0) {
            p.rev[2 * n] = i - 1;
            p.rev[2 * n + 1] = j - 1;
            ++n;
            int code;
            if (i == 0) code = 2;                                                  // trace[0, :] = 2
            else if (j == 0) code = 1;                                             // trace[:, 0] = 1
            else {
                if (wi != i - 1 || wj != (j - 1) >> 4) {
                    wi = i - 1; wj = (j - 1) >> 4;
                    word = p.trace[(int64_t)wi * words + wj];
                }
                code = (word >> (2 * ((j - 1) & 15))) & 3;
            }
            if (code == 0) { --i; --j; }
            else if (code == 1) --i;
            else --j;
        }
        *p.path_len = n;
        n_path = n;
    }
    __threadfence_block();
    __syncthreads();
    const int n = n_path;
    for (int k = r; k < n; k += 256) {
        p.path[2 * k] = p.rev[2 * (n - 1 - k)];
        p.path[2 * k + 1] = p.rev[2 * (n - 1 - k) + 1];
    }
}

size_t dtw_item_bytes(int N, int M) {
    const size_t trace = (size_t)N * ((M + 15) / 16) * 4, rev = (size_t)(N + M) * 8;
    return (trace + rev + 255) / 256 * 256;
}

}  // namespace

extern "C" size_t hirest_whisper_alignment_workspace_bytes(int32_t n_sel, int32_t T, int32_t n_keys) {
    if (n_sel <= 0 || T <= 0 || n_keys <= 0) return 0;
    return (size_t)n_sel * T * n_keys * sizeof(float);
}

extern "C" int hirest_median_filter_mean_f32(const float* w, int32_t n_sel, int32_t T, int32_t n_keys, int32_t width, int32_t row0, int32_t n_rows,
                                             float* out, void* stream) {
    if (!w || !out || n_sel <= 0 || T <= 0 || n_keys <= 0 || row0 < 0 || n_rows <= 0 || (int64_t)row0 + n_rows > T) return HIREST_E_BADARG;
    if (width < 1 || width > MWIDTH_MAX || width % 2 == 0) return HIREST_E_BADARG;
    const int n_tiles = (n_keys + MTILE - 1) / MTILE;
    if ((int64_t)n_rows * n_tiles > 0x7fffffffll) return HIREST_E_SHAPE;
    hipLaunchKernelGGL(align_median_mean_kernel, dim3(n_rows * n_tiles), dim3(MTILE), 0, reinterpret_cast<hipStream_t>(stream), w, (int)n_sel, (int)T,
                       (int)n_keys, (int)width, (int)row0, out, n_tiles);
    return hirest_launch_status();
}

extern "C" int hirest_whisper_alignment_matrix(const float* const* q, int64_t ldq, const float* const* kv, int32_t layers, int32_t heads, int32_t Tk,
                                               const int32_t* sel, int32_t n_sel, int32_t T, int32_t n_keys, float qk_scale, int32_t medfilt_width,
                                               int32_t row0, int32_t n_rows, float* matrix, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !kv || !sel || !matrix || !workspace || layers <= 0 || heads <= 0 || n_sel <= 0 || T <= 0 || Tk <= 0) return HIREST_E_BADARG;
    if (n_keys <= 0 || n_keys > Tk || row0 < 0 || n_rows <= 0 || (int64_t)row0 + n_rows > T) return HIREST_E_BADARG;
    if (medfilt_width < 1 || medfilt_width > MWIDTH_MAX || medfilt_width % 2 == 0) return HIREST_E_BADARG;
    if (heads > AHEADS || ldq < (int64_t)heads * 64 || n_sel > 32767) return HIREST_E_SHAPE;
    for (int s = 0; s < n_sel; ++s)
        if (sel[2 * s] < 0 || sel[2 * s] >= layers || sel[2 * s + 1] < 0 || sel[2 * s + 1] >= heads) return HIREST_E_BADARG;
    for (int l = 0; l < layers; ++l) {
        bool used = false;
        for (int s = 0; s < n_sel; ++s) used |= sel[2 * s] == l;
        if (!used) continue;
        if (!q[l] || !kv[l]) return HIREST_E_BADARG;
        if ((reinterpret_cast<uintptr_t>(kv[l]) & 15) != 0) return HIREST_E_SHAPE;
    }
    if (workspace_bytes < hirest_whisper_alignment_workspace_bytes(n_sel, T, n_keys)) return HIREST_E_WORKSPACE;
    const int nchunk = (n_keys + ACH - 1) / ACH;
    const int64_t rows = (int64_t)n_sel * T;
    if ((int64_t)AHEADS * nchunk > 0x7fffffffll || (rows + 3) / 4 > 0x7fffffffll || ((int64_t)n_sel * n_keys + 255) / 256 > 0x7fffffffll)
        return HIREST_E_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* w = reinterpret_cast<float*>(workspace);
    for (int l = 0; l < layers; ++l) {
        AlignLayer p;
        p.n_heads = 0;
        for (int s = 0; s < n_sel; ++s)
            if (sel[2 * s] == l) {
                if (p.n_heads == AHEADS) return HIREST_E_SHAPE;                    // (a pair listed twice, past every head of the layer)
                p.head[p.n_heads] = (int16_t)sel[2 * s + 1];
                p.sel[p.n_heads++] = (int16_t)s;
            }
        if (p.n_heads == 0) continue;
        for (int e = p.n_heads; e < AHEADS; ++e) p.head[e] = p.sel[e] = 0;
        p.q = q[l]; p.ldq = ldq; p.kv = kv[l]; p.ldkv = 2 * (int64_t)heads * 64;
        p.T = T; p.n_keys = n_keys; p.nchunk = nchunk; p.scale = 0.125f * qk_scale; p.w = w;
        hipLaunchKernelGGL(align_scores_kernel, dim3(p.n_heads * nchunk), dim3(256), 0, st, p);
    }
    hipLaunchKernelGGL(align_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, w, rows, (int)n_keys);
    hipLaunchKernelGGL(align_normalize_kernel, dim3((unsigned)(((int64_t)n_sel * n_keys + 255) / 256)), dim3(256), 0, st, w, (int)n_sel, (int)T, (int)n_keys);
    const int status = hirest_launch_status();
    if (status) return status;
    return hirest_median_filter_mean_f32(w, n_sel, T, n_keys, medfilt_width, row0, n_rows, matrix, stream);
}

extern "C" size_t hirest_dtw_workspace_bytes(const hirest_dtw_problem* problems, int32_t n_problems) {
    if (!problems || n_problems <= 0) return 0;
    size_t total = 0;
    for (int i = 0; i < n_problems; ++i) {
        if (problems[i].N < 1 || problems[i].N > HIREST_DTW_MAX_N || problems[i].M < 1 || problems[i].M > HIREST_DTW_MAX_M) return 0;
        total += dtw_item_bytes(problems[i].N, problems[i].M);
    }
    return total;
}

extern "C" int hirest_dtw_f32(const hirest_dtw_problem* problems, int32_t n_problems, void* workspace, size_t workspace_bytes, void* stream) {
    if (!problems || n_problems <= 0 || !workspace) return HIREST_E_BADARG;
    for (int i = 0; i < n_problems; ++i) {
        const hirest_dtw_problem& q = problems[i];
        if (!q.x || !q.path || !q.path_len || q.N < 1 || q.N > HIREST_DTW_MAX_N || q.M < 1 || q.M > HIREST_DTW_MAX_M) return HIREST_E_BADARG;
        if (q.ldx < q.M || (q.cost && q.ldc < q.M)) return HIREST_E_BADARG;
    }
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return HIREST_E_SHAPE;
    if (workspace_bytes < hirest_dtw_workspace_bytes(problems, n_problems)) return HIREST_E_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    for (int i0 = 0; i0 < n_problems; i0 += DTW_BATCH) {
        DtwBatch b = {};
        const int n = n_problems - i0 < DTW_BATCH ? n_problems - i0 : DTW_BATCH;
        for (int i = 0; i < n; ++i) {
            const hirest_dtw_problem& q = problems[i0 + i];
            DtwItem& it = b.item[i];
            it.x = q.x; it.ldx = q.ldx; it.cost = q.cost; it.ldc = q.ldc; it.path = q.path; it.path_len = q.path_len;
            it.N = q.N; it.M = q.M; it.negate = q.negate != 0;
            it.trace = reinterpret_cast<uint32_t*>(ws);
            it.rev = reinterpret_cast<int32_t*>(ws + (size_t)q.N * ((q.M + 15) / 16) * 4);
            ws += dtw_item_bytes(q.N, q.M);
        }
        hipLaunchKernelGGL(dtw_kernel, dim3(n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), b);
    }
    return hirest_launch_status();
}
