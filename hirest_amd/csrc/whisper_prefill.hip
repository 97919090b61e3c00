// Whisper's prompt prefill for all windows of a decoding loop in one call.  The prompts of the loop's windows, each of
// its own length and each against its own window's cross keys / values, run as packed rows [N, .] through the exact-fp32 GEMMs in
// hirest_whisper_decode_step's per-layer order; the five kernels here are what is ragged about that: the embedding with a position
// per row, causal self-attention and cross-attention per sequence (attention_f32.h's body, so a query has the bits of
// hirest_attention_f32_qkv at B = 1), the scatter of a prompt's keys / values into its window's candidate rows of the caches, and the
// gather of the one or two rows per sequence the LM head is asked for.  A launch takes its sequences by value, SEQ_BATCH at a time:
// nothing is copied to the device and nothing here reads back.  No atomics: a run gives the same bits as the last one.
#include "common.h"
#include "attention_f32.h"
#include "whisper_shared.h"
#include <vector>

namespace {

constexpr int SEQ_BATCH = 64;

struct Seq { int32_t offset, length, window, first_row, n_rows; };
struct SeqBatch { Seq s[SEQ_BATCH]; };

// x[offset_s + j] = tok_emb[ids[offset_s + j]] + pos_emb[j]: hirest_embedding_fwd_f32's one addition, four columns at a time.
// grid (blocks over the longest sequence's float4s, sequence).  An id outside the table is clamped, never an address.
__global__ __launch_bounds__(256) void prefill_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                           const float* __restrict__ pos, float* __restrict__ x, int D4, int vocab,
                                                           SeqBatch b) {
    const Seq& s = b.s[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = i / D4, d = i - j * D4;
    if (j >= s.length) return;
    const int64_t n = (int64_t)s.offset + j;
    int id = ids[n];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const f32x4 a = reinterpret_cast<const f32x4*>(tok)[(int64_t)id * D4 + d], p = reinterpret_cast<const f32x4*>(pos)[(int64_t)j * D4 + d];
    reinterpret_cast<f32x4*>(x)[n * D4 + d] = a + p;
}

// Causal self-attention of every sequence over its own packed rows.  grid (query blocks of the longest sequence * H, sequence);
// NW = waves per block, chosen per launch — a query's bits do not depend on it (attention_f32.h).
template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 1 ? 1 : 3) void attention_f32_ragged_causal_kernel(
        const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, const float* __restrict__ v, int64_t ldkv,
        float* __restrict__ out, int H, float scale, float add_const, float causal_penalty, int qblocks, SeqBatch b) {
    const Seq& s = b.s[blockIdx.y];
    const int h = blockIdx.x / qblocks, qb = blockIdx.x - h * qblocks;
    const int T = s.length;
    if (qb * 32 * NW >= T) return;                                // (block-uniform)
    const int64_t row0 = s.offset;
    attention_f32_block<64, NW>(q + row0 * ldq + h * 64, ldq, k + row0 * ldkv + h * 64, v + row0 * ldkv + h * 64, ldkv, out, row0, H * 64,
                                h * 64, T, T, qb, 64, scale, add_const, causal_penalty);
}

// Cross-attention: sequence s's packed query rows against the key | value rows [Tk, 2 H 64] of its window, at kv + window *
// window_stride.  Sequences may share a window, in any order.
template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 1 ? 1 : 3) void attention_f32_ragged_cross_kernel(
        const float* __restrict__ q, int64_t ldq, const float* __restrict__ kv, int64_t ldkv, int64_t window_stride, int Tk,
        float* __restrict__ out, int H, float scale, float add_const, int qblocks, SeqBatch b) {
    const Seq& s = b.s[blockIdx.y];
    const int h = blockIdx.x / qblocks, qb = blockIdx.x - h * qblocks;
    if (qb * 32 * NW >= s.length) return;                         // (block-uniform)
    const int64_t row0 = s.offset;
    const float* kbase = kv + (int64_t)s.window * window_stride + h * 64;
    attention_f32_block<64, NW>(q + row0 * ldq + h * 64, ldq, kbase, kbase + H * 64, ldkv, out, row0, H * 64, h * 64, s.length, Tk, qb, 64,
                                scale, add_const, 0.f);
}

// Position j of sequence s's keys and values -> position j of cache rows first_row .. first_row + n_rows - 1 of [R, T_max, D], as
// 16-byte vectors.  grid (positions of the longest sequence, sequence): nothing at a position >= length or in a row outside the
// sequence's range is written.
__global__ __launch_bounds__(256) void prefill_scatter_kernel(const float* __restrict__ k, const float* __restrict__ v, int64_t ld,
                                                             float* __restrict__ k_cache, float* __restrict__ v_cache, int T_max, int D4,
                                                             SeqBatch b) {
    const Seq& s = b.s[blockIdx.y];
    const int j = blockIdx.x;
    if (j >= s.length) return;
    const float* ks = k + ((int64_t)s.offset + j) * ld;
    const float* vs = v + ((int64_t)s.offset + j) * ld;
    for (int i = threadIdx.x; i < s.n_rows * D4; i += 256) {
        const int g = i / D4, d = i - g * D4;
        const int64_t dst = (((int64_t)s.first_row + g) * T_max + j) * D4 + d;
        reinterpret_cast<f32x4*>(k_cache)[dst] = reinterpret_cast<const f32x4*>(ks)[d];
        reinterpret_cast<f32x4*>(v_cache)[dst] = reinterpret_cast<const f32x4*>(vs)[d];
    }
}

// out[i] = x[row[i]]: the rows the final LayerNorm and the LM head are asked for
struct RowList { int32_t row[2 * SEQ_BATCH]; };
__global__ __launch_bounds__(256) void prefill_gather_kernel(const float* __restrict__ x, float* __restrict__ out, int D4, RowList r) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D4) return;
    reinterpret_cast<f32x4*>(out)[(int64_t)blockIdx.y * D4 + d] = reinterpret_cast<const f32x4*>(x)[(int64_t)r.row[blockIdx.y] * D4 + d];
}

#define CK(call) do { if (int e_ = (call)) return e_; } while (0)

// What every entry point asks of its sequence table; the caller says which fields it uses (n_windows / R < 0: not that one).
// Packed ranges tile [0, N) in order; lengths in [1, max_len]; windows in [0, n_windows); row ranges inside [0, R), disjoint.
int check_seqs(const hirest_whisper_prefill_seq* seqs, int n_seq, int max_len, int n_windows, int R, int64_t* n_rows_packed, int* longest) {
    if (!seqs || n_seq <= 0 || max_len <= 0) return HIREST_E_BADARG;
    int64_t next = 0;
    int lmax = 0;
    for (int i = 0; i < n_seq; ++i) {
        const hirest_whisper_prefill_seq& s = seqs[i];
        if (s.length < 1 || s.length > max_len || s.offset != next) return HIREST_E_BADARG;
        next += s.length;
        if (next > 0x7fffffffll) return HIREST_E_BADARG;
        lmax = s.length > lmax ? s.length : lmax;
        if (n_windows >= 0 && (s.window < 0 || s.window >= n_windows)) return HIREST_E_BADARG;
        if (s.sot_index >= s.length || (s.sot_index >= 0 && s.sot_index == s.length - 1)) return HIREST_E_BADARG;
        if (R >= 0) {
            if (s.first_row < 0 || s.n_rows < 1 || (int64_t)s.first_row + s.n_rows > R) return HIREST_E_BADARG;
            for (int j = 0; j < i; ++j)
                if (s.first_row < seqs[j].first_row + seqs[j].n_rows && seqs[j].first_row < s.first_row + s.n_rows) return HIREST_E_BADARG;
        }
    }
    *n_rows_packed = next;
    *longest = lmax;
    return 0;
}

int fill_batch(SeqBatch& b, const hirest_whisper_prefill_seq* seqs, int i0, int n_seq) {
    const int n = n_seq - i0 < SEQ_BATCH ? n_seq - i0 : SEQ_BATCH;
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        const hirest_whisper_prefill_seq& s = seqs[i0 + i];
        b.s[i] = Seq{s.offset, s.length, s.window, s.first_row, s.n_rows};
        longest = s.length > longest ? s.length : longest;
    }
    for (int i = n; i < SEQ_BATCH; ++i) b.s[i] = Seq{0, 0, 0, 0, 0};
    return longest;
}

// waves per block for a launch whose longest sequence has `longest` queries: hirest_attention_f32_qkv's rule
inline int waves_per_block(int longest) {
    const int waves = (longest + 31) / 32;
    return longest <= 64 ? 1 : ((waves + 2) / 3 * 3 < (waves + 3) / 4 * 4 ? 3 : 4);
}

// One launch per SEQ_BATCH sequences of a ragged attention form: KERNEL<NW> with NW chosen for the batch's longest sequence, called as
// kernel(front..., qblocks, batch) on a grid of (query blocks * H, sequences).
#define LAUNCH_RAGGED(KERNEL, ...)                                                                                                   \
    for (int i0 = 0; i0 < n_seq; i0 += SEQ_BATCH) {                                                                                  \
        SeqBatch b;                                                                                                                  \
        const int longest = fill_batch(b, seqs, i0, n_seq), n = n_seq - i0 < SEQ_BATCH ? n_seq - i0 : SEQ_BATCH;                     \
        const int nw = waves_per_block(longest), qblocks = (longest + 32 * nw - 1) / (32 * nw);                                      \
        const dim3 grid(qblocks * H, n);                                                                                             \
        if (nw == 1) hipLaunchKernelGGL(KERNEL<1>, grid, dim3(64), 0, st, __VA_ARGS__, qblocks, b);                                  \
        else if (nw == 3) hipLaunchKernelGGL(KERNEL<3>, grid, dim3(192), 0, st, __VA_ARGS__, qblocks, b);                            \
        else hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, st, __VA_ARGS__, qblocks, b);                                         \
    }

int launch_causal(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, float* out, const hirest_whisper_prefill_seq* seqs,
                  int n_seq, int H, float scale, float add_const, float causal_penalty, hipStream_t st) {
    LAUNCH_RAGGED(attention_f32_ragged_causal_kernel, q, ldq, k, v, ldkv, out, H, scale, add_const, causal_penalty)
    return hirest_launch_status();
}

int launch_cross(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int64_t window_stride, int Tk, float* out,
                 const hirest_whisper_prefill_seq* seqs, int n_seq, int H, float scale, float add_const, hipStream_t st) {
    LAUNCH_RAGGED(attention_f32_ragged_cross_kernel, q, ldq, kv, ldkv, window_stride, Tk, out, H, scale, add_const)
    return hirest_launch_status();
}

int launch_scatter(const float* k, const float* v, int64_t ld, float* k_cache, float* v_cache, int T_max, int D,
                   const hirest_whisper_prefill_seq* seqs, int n_seq, hipStream_t st) {
    for (int i0 = 0; i0 < n_seq; i0 += SEQ_BATCH) {
        SeqBatch b;
        const int longest = fill_batch(b, seqs, i0, n_seq), n = n_seq - i0 < SEQ_BATCH ? n_seq - i0 : SEQ_BATCH;
        hipLaunchKernelGGL(prefill_scatter_kernel, dim3(longest, n), dim3(256), 0, st, k, v, ld, k_cache, v_cache, T_max, D / 4, b);
    }
    return hirest_launch_status();
}

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t max2(size_t a, size_t b) { return a > b ? a : b; }

struct Ws { size_t x, a, b, ln, qkv, ctx, mid, gat, gemm, gemm_bytes, total; };
Ws plan(const hirest_whisper_decoder* d, int N, int n_seq) {
    Ws w; size_t off = 0;
    const size_t D = d->hidden;
    w.x = off; off += al((size_t)N * D * 4);
    w.a = off; off += al((size_t)N * D * 4);
    w.b = off; off += al((size_t)N * D * 4);
    w.ln = off; off += al((size_t)N * D * 4);
    w.qkv = off; off += al((size_t)N * 3 * D * 4);
    w.ctx = off; off += al((size_t)N * D * 4);
    w.mid = off; off += al((size_t)N * d->inter * 4);
    w.gat = off; off += al((size_t)2 * n_seq * D * 4);            // the gathered rows: every sequence's last, then the sot rows asked for
    // the split form of hirest_gemm_f32_ws, where one of the layer's products takes it (same bits as the plain form)
    w.gemm_bytes = max2(max2(hirest_gemm_f32_workspace_bytes(N, 3 * (int)D, (int)D), hirest_gemm_f32_workspace_bytes(N, (int)D, (int)D)),
                        max2(hirest_gemm_f32_workspace_bytes(N, d->inter, (int)D), hirest_gemm_f32_workspace_bytes(N, (int)D, d->inter)));
    w.gemm = off; off += al(w.gemm_bytes);
    w.total = off;
    return w;
}

int gemm(const float* A, int K, const float* W, const float* bias, const float* resid, float* out, int M, int N, int act, void* gws, size_t gws_bytes,
         void* stream) {
    return hirest_gemm_f32_ws(A, K, W, K, bias, resid, N, nullptr, 0, out, N, M, N, K, act, gws, gws_bytes, stream);
}

// act(LayerNorm(X) W^T + bias): inside one GEMM where hirest_gemm_f32_ln has a form for the shape, else two calls — the same bits.
// The routing is whisper_shared.h's, as the decoding step's.
int ln_gemm(const float* X, const float* g, const float* b, float* ln_scratch, const float* W, const float* bias, float* out, int R, int N,
            int K, int act, void* gws, size_t gws_bytes, void* stream) {
    const float eps = 1e-5f;
    if (whisper_ln_gemm_fused(R, N, K))
        return hirest_gemm_f32_ln(X, K, nullptr, nullptr, nullptr, g, b, eps, nullptr, 0, W, K, bias, nullptr, 0, out, N, R, N, K, act, stream);
    CK(hirest_layernorm(X, K, nullptr, g, b, eps, ln_scratch, K, 1, R, K, stream));
    return gemm(ln_scratch, K, W, bias, nullptr, out, R, N, act, gws, gws_bytes, stream);
}

inline bool bad_decoder(const hirest_whisper_decoder* d) {
    return !d || !d->layer || !d->tok_emb || !d->pos_emb || !d->ln_g || !d->ln_b || !d->lm_b || d->layers <= 0 || d->max_pos <= 0;
}

}  // namespace

extern "C" int hirest_embedding_varlen_fwd_f32(const int32_t* ids, const float* table, const float* pos, float* out, int32_t vocab, int32_t max_pos,
                                               int32_t D, const hirest_whisper_prefill_seq* seqs, int32_t n_seq, void* stream) {
    if (!ids || !table || !pos || !out || vocab <= 0 || max_pos <= 0 || D <= 0 || D % 4 != 0) return HIREST_E_BADARG;
    int64_t N; int longest;
    CK(check_seqs(seqs, n_seq, max_pos, -1, -1, &N, &longest));
    for (int i0 = 0; i0 < n_seq; i0 += SEQ_BATCH) {
        SeqBatch b;
        const int lmax = fill_batch(b, seqs, i0, n_seq), n = n_seq - i0 < SEQ_BATCH ? n_seq - i0 : SEQ_BATCH;
        hipLaunchKernelGGL(prefill_embed_kernel, dim3((unsigned)(((int64_t)lmax * (D / 4) + 255) / 256), n), dim3(256), 0,
                           reinterpret_cast<hipStream_t>(stream), ids, table, pos, out, D / 4, (int)vocab, b);
    }
    return hirest_launch_status();
}

extern "C" int hirest_attention_f32_varlen_causal(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, float* out,
                                                  const hirest_whisper_prefill_seq* seqs, int32_t n_seq, int32_t H, float scale, float add_const,
                                                  float causal_penalty, void* stream) {
    if (!q || !k || !v || !out || H <= 0) return HIREST_E_BADARG;
    int64_t N; int longest;
    CK(check_seqs(seqs, n_seq, 0x7fffffff, -1, -1, &N, &longest));
    if (ldq % 4 != 0 || ldkv % 4 != 0 || ldq < (int64_t)H * 64 || ldkv < (int64_t)H * 64) return HIREST_E_SHAPE;
    if (((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) return HIREST_E_SHAPE;
    return launch_causal(q, ldq, k, v, ldkv, out, seqs, n_seq, H, scale, add_const, causal_penalty, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hirest_attention_f32_varlen_cross(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int64_t window_stride, int32_t n_windows,
                                                 int32_t Tk, float* out, const hirest_whisper_prefill_seq* seqs, int32_t n_seq, int32_t H, float scale,
                                                 float add_const, void* stream) {
    if (!q || !kv || !out || H <= 0 || Tk <= 0 || n_windows <= 0) return HIREST_E_BADARG;
    int64_t N; int longest;
    CK(check_seqs(seqs, n_seq, 0x7fffffff, n_windows, -1, &N, &longest));
    if (ldq % 4 != 0 || ldkv % 4 != 0 || window_stride % 4 != 0 || ldq < (int64_t)H * 64 || ldkv < 2 * (int64_t)H * 64 ||
        (n_windows > 1 && window_stride < (int64_t)Tk * ldkv))
        return HIREST_E_SHAPE;
    if (((reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) return HIREST_E_SHAPE;
    return launch_cross(q, ldq, kv, ldkv, window_stride, Tk, out, seqs, n_seq, H, scale, add_const, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hirest_whisper_prefill_scatter(const float* k, const float* v, int64_t ld, float* k_cache, float* v_cache, int32_t R, int32_t T_max,
                                              int32_t D, const hirest_whisper_prefill_seq* seqs, int32_t n_seq, void* stream) {
    if (!k || !v || !k_cache || !v_cache || R <= 0 || T_max <= 0 || D <= 0 || D % 4 != 0) return HIREST_E_BADARG;
    int64_t N; int longest;
    CK(check_seqs(seqs, n_seq, T_max, -1, R, &N, &longest));
    if (ld % 4 != 0 || ld < D) return HIREST_E_SHAPE;
    if (((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15) != 0)
        return HIREST_E_SHAPE;
    return launch_scatter(k, v, ld, k_cache, v_cache, T_max, D, seqs, n_seq, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t hirest_whisper_prefill_workspace_bytes(const hirest_whisper_decoder* d, int32_t n_rows_packed, int32_t n_seq) {
    if (!d || n_rows_packed <= 0 || n_seq <= 0 || d->hidden <= 0 || d->inter <= 0) return 0;
    return plan(d, n_rows_packed, n_seq).total;
}

extern "C" int hirest_whisper_prefill_rows(const hirest_whisper_decoder* d, int32_t n_seq, const hirest_whisper_prefill_seq* seqs, const int32_t* ids,
                                           float* const* self_k, float* const* self_v, int32_t R, int32_t T_max, const float* const* cross_kv,
                                           int32_t n_windows, int32_t Tk, float* logits_last, float* logits_sot, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    if (bad_decoder(d) || !seqs || !ids || !self_k || !self_v || !cross_kv || !logits_last || !workspace || n_seq <= 0 || R <= 0 || T_max <= 0 ||
        Tk <= 0 || n_windows <= 0)
        return HIREST_E_BADARG;
    int64_t N64; int longest;
    CK(check_seqs(seqs, n_seq, d->max_pos < T_max ? d->max_pos : T_max, n_windows, R, &N64, &longest));
    int n_sot = 0;
    for (int i = 0; i < n_seq; ++i) n_sot += seqs[i].sot_index >= 0;
    if (n_sot && !logits_sot) return HIREST_E_BADARG;
    for (int i = 0; i < d->layers; ++i)
        if (!self_k[i] || !self_v[i] || !cross_kv[i]) return HIREST_E_BADARG;
    const int D = d->hidden, H = d->heads, I = d->inter, Vp = d->vocab_padded, N = (int)N64;
    if (H <= 0 || D != H * 64 || I <= 0 || I % 16 != 0 || Vp <= 0 || Vp % 4 != 0) return HIREST_E_SHAPE;
    const Ws w = plan(d, N, n_seq);
    if (workspace_bytes < w.total) return HIREST_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return HIREST_E_SHAPE;
    for (int i = 0; i < d->layers; ++i)
        if (((reinterpret_cast<uintptr_t>(self_k[i]) | reinterpret_cast<uintptr_t>(self_v[i]) | reinterpret_cast<uintptr_t>(cross_kv[i])) & 15) != 0)
            return HIREST_E_SHAPE;
    char* base = static_cast<char*>(workspace);
    float* x = reinterpret_cast<float*>(base + w.x);
    float* a = reinterpret_cast<float*>(base + w.a);
    float* b = reinterpret_cast<float*>(base + w.b);
    float* ln = reinterpret_cast<float*>(base + w.ln);
    float* qkv = reinterpret_cast<float*>(base + w.qkv);
    float* ctx = reinterpret_cast<float*>(base + w.ctx);
    float* mid = reinterpret_cast<float*>(base + w.mid);
    float* gat = reinterpret_cast<float*>(base + w.gat);
    void* gws = w.gemm_bytes ? base + w.gemm : nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float scale = 0.125f;                                   // 64^-0.5: Whisper scales q and k by 64^-0.25 each
    const float causal = -1.0e30f;                                // whisper.py's _CAUSAL_PENALTY: exp() of it is exactly 0
    CK(hirest_embedding_varlen_fwd_f32(ids, d->tok_emb, d->pos_emb, x, Vp, d->max_pos, D, seqs, n_seq, stream));
    for (int i = 0; i < d->layers; ++i) {
        const hirest_whisper_layer& L = d->layer[i];
        CK(ln_gemm(x, L.attn_ln_g, L.attn_ln_b, ln, L.qkv_w, L.qkv_b, qkv, N, 3 * D, D, 0, gws, w.gemm_bytes, stream));
        CK(launch_causal(qkv, 3 * D, qkv + D, qkv + 2 * D, 3 * D, ctx, seqs, n_seq, H, scale, 0.f, causal, s));
        CK(launch_scatter(qkv + D, qkv + 2 * D, 3 * D, self_k[i], self_v[i], T_max, D, seqs, n_seq, s));
        CK(gemm(ctx, D, L.so_w, L.so_b, x, a, N, D, 0, gws, w.gemm_bytes, stream));
        CK(ln_gemm(a, L.cross_ln_g, L.cross_ln_b, ln, L.cq_w, L.cq_b, qkv, N, D, D, 0, gws, w.gemm_bytes, stream));
        CK(launch_cross(qkv, D, cross_kv[i], 2 * D, (int64_t)Tk * 2 * D, Tk, ctx, seqs, n_seq, H, scale, 0.f, s));
        CK(gemm(ctx, D, L.co_w, L.co_b, a, b, N, D, 0, gws, w.gemm_bytes, stream));
        CK(ln_gemm(b, L.mlp_ln_g, L.mlp_ln_b, ln, L.fc1_w, L.fc1_b, mid, N, I, D, 1, gws, w.gemm_bytes, stream));
        CK(gemm(mid, I, L.fc2_w, L.fc2_b, b, x, N, D, 0, gws, w.gemm_bytes, stream));
    }
    // the rows the loop reads: every sequence's last position, then (compacted, in sequence order) the sot positions asked for
    std::vector<int32_t> rows;
    rows.reserve(n_seq + n_sot);
    for (int i = 0; i < n_seq; ++i) rows.push_back(seqs[i].offset + seqs[i].length - 1);
    for (int i = 0; i < n_seq; ++i)
        if (seqs[i].sot_index >= 0) rows.push_back(seqs[i].offset + seqs[i].sot_index);
    for (size_t r0 = 0; r0 < rows.size(); r0 += 2 * SEQ_BATCH) {
        RowList rl = {};
        const int n = (int)(rows.size() - r0 < 2 * SEQ_BATCH ? rows.size() - r0 : 2 * SEQ_BATCH);
        for (int i = 0; i < n; ++i) rl.row[i] = rows[r0 + i];
        hipLaunchKernelGGL(prefill_gather_kernel, dim3((D / 4 + 255) / 256, n), dim3(256), 0, s, x, gat + (int64_t)r0 * D, D / 4, rl);
    }
    // (b is free again: the LayerNorm scratch of the head's two-call form)
    CK(ln_gemm(gat, d->ln_g, d->ln_b, b, d->tok_emb, d->lm_b, logits_last, n_seq, Vp, D, 0, nullptr, 0, stream));
    // logits_sot row s is written only where sequence s asked: one product per run of consecutive sequences that did
    for (int i = 0, c = 0; i < n_seq;) {
        if (seqs[i].sot_index < 0) { ++i; continue; }
        int j = i;
        while (j < n_seq && seqs[j].sot_index >= 0) ++j;
        CK(ln_gemm(gat + (int64_t)(n_seq + c) * D, d->ln_g, d->ln_b, b, d->tok_emb, d->lm_b, logits_sot + (int64_t)i * Vp, j - i, Vp, D, 0, nullptr, 0,
                   stream));
        c += j - i;
        i = j;
    }
    return hirest_launch_status();
}
