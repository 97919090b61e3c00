// Whisper's text decoder on gfx950: the two kernels a decoded token needs that the tree did not have — one-query
// cross-attention over a long, shared key set, split over keys, and the whole tail of a sampling step (logit filters, log_softmax, the
// pick, the row's bookkeeping) with its state on the device — and the C-side step that strings them together with the exact-fp32
// GEMMs.  The in-place self-attention form lives beside the kernel it shares its body with (joint.hip).  The `_rows` entry points
//  are the same step and tail for rows of several windows, each with its own position, step, temperature and seed in a
// device record (hirest_whisper_row_ctl).  Language detection is one per-row step at position 0 and the small softmax
// over the language tokens' columns below (whisper_language_tail_kernel).
#include "common.h"
#include "whisper_shared.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// Cross-attention, one query per row.  Work is cut as (window, head, chunk of XCH keys); XCH is a constant, so the chunking of a
// row's keys depends on Tk alone.  A block of four waves stages its chunk of K and V for its head in LDS once — with vector loads:
// the K rows are padded to 68 floats so that the lane = key float4 reads of the score pass spread over the banks, and LDS-DMA
// can only lay a wave's 1024 bytes down contiguously — and serves every row that attends to its window from it (the n-th such row
// goes to wave n mod 4; a row's arithmetic does not depend on the wave that runs it).  Per (row, head, chunk) it leaves a record of
// XREC floats: 64 un-normalised outputs, the chunk's maximum score and the sum of its exponentials.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int XCH = 64, XREC = 68, XKLD = 68;

struct XDec {
    const float* q; int64_t ldq;
    const float* kv; int64_t ldkv, window_stride;
    const int32_t* row_window;
    int R, H, Tk, nchunk, n_windows;
    float scale;
    float* part;
    float* out; int64_t ldo;
};

__device__ __forceinline__ float bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

__global__ __launch_bounds__(256) void cross_partial_kernel(XDec p) {
    __shared__ __attribute__((aligned(16))) float Ks[XCH * XKLD];
    __shared__ __attribute__((aligned(16))) float Vs[XCH * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x % p.nchunk, h = (blockIdx.x / p.nchunk) % p.H, w = blockIdx.x / (p.nchunk * p.H);
    int any = 0;
    for (int r = 0; r < p.R; ++r) any |= p.row_window[r] == w;
    if (!any) return;                                             // (block-uniform) no row of this call attends to the window
    const int k0 = c * XCH;
    const float* base = p.kv + (int64_t)w * p.window_stride + h * 64;
    f32x4 kreg[4], vreg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                 // keys past Tk re-read key Tk - 1; their scores are masked below
        const int idx = tid + 256 * i, key = k0 + (idx >> 4), kk = key < p.Tk ? key : p.Tk - 1;
        const float* row = base + (int64_t)kk * p.ldkv + 4 * (idx & 15);
        kreg[i] = *reinterpret_cast<const f32x4*>(row);
        vreg[i] = *reinterpret_cast<const f32x4*>(row + p.H * 64);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        *reinterpret_cast<f32x4*>(Ks + (idx >> 4) * XKLD + 4 * (idx & 15)) = kreg[i];
        *reinterpret_cast<f32x4*>(Vs + (idx >> 4) * 64 + 4 * (idx & 15)) = vreg[i];
    }
    __syncthreads();
    int cnt = 0;
    for (int r = 0; r < p.R; ++r) {
        if (p.row_window[r] != w) continue;
        if ((cnt++ & 3) != wave) continue;                        // (wave-uniform)
        const float qv = p.q[(int64_t)r * p.ldq + h * 64 + lane];
        float st = 0.f;                                           // lane = key k0 + lane: q . k, d = 0 .. 63 in order
#pragma unroll
        for (int c4 = 0; c4 < 16; ++c4) {
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(Ks + lane * XKLD + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) st = __builtin_fmaf(k4[e], bcast(qv, 4 * c4 + e), st);
        }
        const float sv = k0 + lane < p.Tk ? st * p.scale : -3.0e38f;
        const float m = wave_max(sv);                             // finite: a chunk holds at least one key
        const float pz = k0 + lane < p.Tk ? expf(sv - m) : 0.f;
        const float l = wave_sum(pz);
        float o = 0.f;                                            // lane = d: keys in ascending order
#pragma unroll
        for (int j = 0; j < XCH; ++j) o = __builtin_fmaf(Vs[j * 64 + lane], bcast(pz, j), o);
        float* rec = p.part + (((int64_t)r * p.H + h) * p.nchunk + c) * XREC;
        rec[lane] = o;
        if (lane == 0) { rec[64] = m; rec[65] = l; }
    }
}

// one wave per (row, head): the row's chunk records in ascending chunk order
__global__ __launch_bounds__(64) void cross_merge_kernel(XDec p) {
    const int lane = threadIdx.x, r = blockIdx.x / p.H, h = blockIdx.x - r * p.H;
    float* orow = p.out + (int64_t)r * p.ldo + h * 64;
    const int w = p.row_window[r];
    if (w < 0 || w >= p.n_windows) { orow[lane] = 0.f; return; }  // no block wrote records for such a row
    const float* rec = p.part + (int64_t)blockIdx.x * p.nchunk * XREC;
    float M = -3.0e38f;
    for (int c = 0; c < p.nchunk; ++c) M = fmaxf(M, rec[c * XREC + 64]);
    float l = 0.f, o = 0.f;
    for (int c = 0; c < p.nchunk; ++c) {
        const float a = expf(rec[c * XREC + 64] - M);
        l = __builtin_fmaf(rec[c * XREC + 65], a, l);
        o = __builtin_fmaf(rec[c * XREC + lane], a, o);
    }
    orow[lane] = o / l;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The tail of a sampling step.  One block of 1024 threads per row, three passes over a row of logits that stays in the L2:
// maxima, sums of exponentials (the text tokens and the timestamp tokens apart, which is what the log-sum-exp rule compares, and at
// the first position the unfiltered row for no_speech_prob), then the pick.  Every reduction has a fixed order: a thread's elements
// in ascending index order, the wave's 64 partial results by xor shuffles, the 16 waves' in wave order.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr float NEG = -3.0e38f;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {           // train.hip's counter-based generator (the splitmix64 finaliser)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t draw_key(uint32_t seed, uint32_t serial) {
    return mix64((((uint64_t)serial << 32) | seed) + 0x9E3779B97F4A7C15ull);
}
__device__ __forceinline__ uint32_t draw_bits(uint64_t key, uint32_t row, uint32_t tok) {     // 24 bits
    return (uint32_t)(mix64(key + (((uint64_t)row << 32) | tok) + 0x9E3779B97F4A7C15ull) >> 40);
}
__device__ __forceinline__ float gumbel(uint32_t bits) {
    const float u = ((float)(bits >> 1) + 0.5f) * (1.0f / 8388608.0f);    // the top 23 bits: (0, 1), every value exact in fp32
    return -logf(-logf(u));
}

struct Rule {                // what a row's history allows, besides the suppress mask
    int first, blank, eot, rules, no_ts, tb, ts_min, ts_max, no_ts_at_all, no_text, text_from;
};
__device__ __forceinline__ bool allowed(const Rule& k, const uint32_t* __restrict__ mask, int v) {
    if (mask[v >> 5] >> (v & 31) & 1u) return false;
    if (k.first && k.blank >= 0 && (v == k.blank || v == k.eot)) return false;
    if (!k.rules) return true;
    if (v == k.no_ts) return false;
    if (v >= k.tb) return !k.no_ts_at_all && v >= k.ts_min && v <= k.ts_max;
    return !k.no_text && v >= k.text_from;
}

__device__ __forceinline__ float block_max(float v, float* sh, int tid) {
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    float m = sh[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) m = fmaxf(m, sh[i]);
    return m;
}
__device__ __forceinline__ float block_sum(float v, float* sh, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    float s = sh[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) s += sh[i];
    return s;
}

// One row that is not completed, by its block: x the row's V logits, st its state on entry (block-uniform), lp_row where its
// log-probabilities go (or null).  The draw is keyed by (seed, serial, draw_row): in a call of one window these are the call's own
// and the row's index, in a call of rows from several windows the row's record supplies them.  Thread 0 stores the new state, the
// pick and the token slot and gets the pick back; every other thread gets -1.
__device__ __forceinline__ int tail_row(const float* __restrict__ x, int V, const hirest_whisper_tail_params& c, float temperature, uint32_t seed,
                                        uint32_t serial, uint32_t draw_row, const hirest_whisper_row_state& st,
                                        hirest_whisper_row_state* __restrict__ state_out, int32_t* __restrict__ next_id,
                                        int32_t* __restrict__ slot, float* __restrict__ lp_row) {
    __shared__ float sh[16];
    __shared__ float best_v[16];
    __shared__ int best_i[16];
    const int tid = threadIdx.x;
    const uint32_t* mask = c.suppress_mask;
    const int tb = c.timestamp_begin;
    Rule k;
    k.first = st.n_sampled == 0; k.blank = c.suppress_blank ? c.blank : -1; k.eot = c.eot; k.rules = c.timestamp_rules; k.no_ts = c.no_timestamps;
    k.tb = tb; k.ts_min = tb; k.ts_max = 0x7fffffff; k.no_ts_at_all = 0; k.no_text = 0; k.text_from = 0;
    if (k.rules) {
        const bool last_ts = st.n_sampled >= 1 && st.last >= tb, pen_ts = st.n_sampled < 2 || st.penult >= tb;
        if (last_ts) { if (pen_ts) k.no_ts_at_all = 1; else k.text_from = c.eot; }     // pairs; after text + timestamp: a timestamp or eot
        if (st.last_timestamp >= 0 && c.monotonic) k.ts_min = last_ts && !pen_ts ? st.last_timestamp : st.last_timestamp + 1;
        if (k.first) { k.no_text = 1; if (c.max_initial_timestamp_index >= 0) k.ts_max = tb + c.max_initial_timestamp_index; }
    }
    const int V4 = V >> 2;
    // pass 1: maxima
    float m_text = NEG, m_ts = NEG, m_raw = NEG;
    for (int i = tid; i < V4; i += 1024) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(x + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 4 * i + e;
            if (v < c.n_vocab) m_raw = fmaxf(m_raw, v4[e]);
            if (allowed(k, mask, v)) { if (v >= tb) m_ts = fmaxf(m_ts, v4[e]); else m_text = fmaxf(m_text, v4[e]); }
        }
    }
    m_text = block_max(m_text, sh, tid); m_ts = block_max(m_ts, sh, tid);
    if (k.first) m_raw = block_max(m_raw, sh, tid);
    const bool has_text = m_text > NEG, has_ts = m_ts > NEG;
    // pass 2: sums of exponentials, each part against its own maximum
    float s_text = 0.f, s_ts = 0.f, s_raw = 0.f;
    for (int i = tid; i < V4; i += 1024) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(x + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 4 * i + e;
            if (k.first && v < c.n_vocab) s_raw += expf(v4[e] - m_raw);
            if (allowed(k, mask, v)) { if (v >= tb) s_ts += expf(v4[e] - m_ts); else s_text += expf(v4[e] - m_text); }
        }
    }
    s_text = block_sum(s_text, sh, tid); s_ts = block_sum(s_ts, sh, tid);
    if (k.first) s_raw = block_sum(s_raw, sh, tid);
    // log-sum-exp of the timestamps above every text token: the text tokens go (the comparison of the two log-probabilities,
    // with the common log-sum-exp taken off both sides)
    const float lse_ts = has_ts ? m_ts + logf(s_ts) : NEG;
    if (k.rules && has_ts && (!has_text || lse_ts > m_text)) k.no_text = 1;
    const bool text_in = has_text && !k.no_text;
    float M, S;                                                   // log-sum-exp of what is left = M + log S
    if (text_in && has_ts) { M = fmaxf(m_text, m_ts); S = s_text * expf(m_text - M) + s_ts * expf(m_ts - M); }
    else if (text_in) { M = m_text; S = s_text; }
    else { M = m_ts; S = s_ts; }
    if (lp_row) {                                                 // log_softmax of the filtered row, -inf where suppressed
        const float logS = logf(S);
        for (int i = tid; i < V4; i += 1024) {
            const f32x4 v4 = *reinterpret_cast<const f32x4*>(x + 4 * i);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = allowed(k, mask, 4 * i + e) ? (v4[e] - M) - logS : -INFINITY;
            *reinterpret_cast<f32x4*>(lp_row + 4 * i) = o;
        }
    }
    // pass 3: the pick — the largest logit (T = 0) or the largest logit / T + Gumbel noise (a categorical draw); the lower index on ties
    const bool sample = temperature > 0.f;
    const uint64_t key = draw_key(seed, serial);
    float bv = NEG; int bi = 0x7fffffff;
    for (int i = tid; i < V4; i += 1024) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(x + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 4 * i + e;
            if (!allowed(k, mask, v)) continue;
            const float s = sample ? v4[e] / temperature + gumbel(draw_bits(key, draw_row, (uint32_t)v)) : v4[e];
            if (s > bv) { bv = s; bi = v; }                       // (ascending v: the first of equals stays)
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
    __syncthreads();
    int pick = -1;
    if (tid == 0) {
        for (int i = 1; i < 16; ++i)
            if (best_v[i] > bv || (best_v[i] == bv && best_i[i] < bi)) { bv = best_v[i]; bi = best_i[i]; }
        hirest_whisper_row_state ns = st;
        pick = bi;
        float lp = 0.f;
        if (pick >= V || !(text_in || has_ts)) pick = c.eot;       // nothing was allowed: end the row (no log-probability to add)
        else lp = (x[pick] - M) - logf(S);
        if (k.first) ns.no_speech_prob = c.no_speech >= 0 ? expf(x[c.no_speech] - m_raw) / s_raw : 0.f;
        ns.sum_logprobs = st.sum_logprobs + lp;                   // the logits' own log-probability (temperature 1), eot's included
        ns.last_logprob = lp;
        if (pick == c.eot) ns.completed = 1;
        else {
            ns.n_sampled = st.n_sampled + 1; ns.penult = st.last; ns.last = pick;
            if (pick >= tb) ns.last_timestamp = pick;
        }
        *state_out = ns;
        *next_id = pick;
        if (slot) *slot = pick;
    }
    return pick;
}

__global__ __launch_bounds__(1024) void whisper_tail_kernel(const float* __restrict__ logits, int64_t ldx, int V, int step, int T_max,
                                                           hirest_whisper_tail_params c, hirest_whisper_row_state* __restrict__ state,
                                                           int32_t* __restrict__ next_ids, int32_t* __restrict__ tokens,
                                                           float* __restrict__ logprobs) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const hirest_whisper_row_state st = state[r];                 // (block-uniform: written only by this block, in an earlier launch)
    int32_t* slot = tokens ? tokens + (int64_t)r * T_max + c.sample_begin + step : nullptr;
    if (st.completed) {
        if (tid == 0) { next_ids[r] = c.eot; if (slot) *slot = c.eot; }
        return;
    }
    tail_row(logits + (int64_t)r * ldx, V, c, c.temperature, c.seed, c.serial, (uint32_t)r, st, state + r, next_ids + r, slot,
             logprobs ? logprobs + (int64_t)r * V : nullptr);
}

// Rows of several windows in one call: step, temperature, seed and the generator's row come from the row's record, and the block
// advances the record after its pick.  A row leaves the loop (position = -1) on eot or when it has made max_steps picks; the latter
// neither completes it nor writes an eot, as a call per window that stops at its last step does not.  An inactive row's block
// returns at once: nothing of the row changes.
__global__ __launch_bounds__(1024) void whisper_tail_rows_kernel(const float* __restrict__ logits, int64_t ldx, int V, int64_t ld_tokens,
                                                                hirest_whisper_tail_params c, hirest_whisper_row_ctl* __restrict__ ctl,
                                                                hirest_whisper_row_state* __restrict__ state, int32_t* __restrict__ next_ids,
                                                                int32_t* __restrict__ tokens, float* __restrict__ logprobs) {
    const int r = blockIdx.x;
    const hirest_whisper_row_ctl rc = ctl[r];                     // (block-uniform, as the state)
    if (rc.position < 0) return;
    const hirest_whisper_row_state st = state[r];
    if (st.completed || rc.step < 0 || rc.step >= rc.max_steps || rc.step >= ld_tokens) {     // no pick to make: the row leaves the loop
        if (threadIdx.x == 0) ctl[r].position = -1;
        return;
    }
    const int pick = tail_row(logits + (int64_t)r * ldx, V, c, rc.temperature, rc.seed, (uint32_t)rc.step, (uint32_t)rc.draw_row, st, state + r,
                              next_ids + r, tokens + (int64_t)r * ld_tokens + rc.step, logprobs ? logprobs + (int64_t)r * V : nullptr);
    if (threadIdx.x == 0) {
        const int step = rc.step + 1;
        ctl[r].step = step;
        ctl[r].position = pick == c.eot || step >= rc.max_steps ? -1 : rc.position + 1;
    }
}

// ((step + 1) << 1) | every row completed, into pinned host memory: the host loop polls the word, no event per step
__global__ __launch_bounds__(64) void whisper_stamp_kernel(const hirest_whisper_row_state* __restrict__ state, int R, int step,
                                                          int32_t* __restrict__ done_host) {
    int all = 1;
    for (int r = threadIdx.x; r < R; r += 64) all &= state[r].completed != 0;
    all = __all(all);
    if (threadIdx.x == 0) *done_host = ((step + 1) << 1) | (all ? 1 : 0);
}

// the same word for a call of rows: ((call + 1) << 1) | no row is active any more
__global__ __launch_bounds__(64) void whisper_stamp_rows_kernel(const hirest_whisper_row_ctl* __restrict__ ctl, int R, int call,
                                                               int32_t* __restrict__ done_host) {
    int none = 1;
    for (int r = threadIdx.x; r < R; r += 64) none &= ctl[r].position < 0;
    none = __all(none);
    if (threadIdx.x == 0) *done_host = ((call + 1) << 1) | (none ? 1 : 0);
}

// the counted form: the call's number is a device word, read and advanced by this one lane — nothing of the launch
// changes from call to call, so a captured sequence of tails stamps 2, 4, 6, ... as it is replayed
__global__ __launch_bounds__(64) void whisper_stamp_rows_counted_kernel(const hirest_whisper_row_ctl* __restrict__ ctl, int R,
                                                                       int32_t* __restrict__ count, int32_t* __restrict__ done_host) {
    int none = 1;
    for (int r = threadIdx.x; r < R; r += 64) none &= ctl[r].position < 0;
    none = __all(none);
    if (threadIdx.x == 0) {
        const int call = *count;
        if (done_host) *done_host = ((call + 1) << 1) | (none ? 1 : 0);
        *count = call + 1;
    }
}

// Language detection: the softmax of a row of logits over the L <= 128 language columns alone, and its argmax.  One
// wave per row; lane l holds table entries l and l + 64.  The maximum is the tail's pick (strict > over ascending ids, then the xor
// tree with the lower id on ties), the sum a lane's two terms in ascending order and then wave_sum's xor tree in double: fixed orders, so a row
// has the same bits whatever else is in the call.  Only the table's columns are read; an id outside [0, V) counts as absent
// (probability 0) and is never an address.
__global__ __launch_bounds__(64) void whisper_language_tail_kernel(const float* __restrict__ logits, int64_t ldx, int V,
                                                                  const int32_t* __restrict__ ids, int L, int32_t* __restrict__ lang_token,
                                                                  float* __restrict__ probs) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* x = logits + (int64_t)r * ldx;
    float v[2];
    bool have[2];
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int j = lane + 64 * e;
        const int id = j < L ? ids[j] : -1;
        have[e] = id >= 0 && id < V;
        v[e] = have[e] ? x[id] : -INFINITY;
        if (have[e] && (bi == 0x7fffffff || v[e] > bv)) { bv = v[e]; bi = id; }      // (ascending ids: the first of equals stays)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    // The denominator and the quotients in double: every quotient carries the denominator's rounding error whole, so a row's sum
    // would miss 1 by what L - 1 fp32 additions lose (3e-7 at L = 100) while a single probability only shows it scaled by itself.
    // Summed in double the sum is exact to fp32, each quotient is rounded once, and a row sums to 1 within those roundings.
    float p[2];
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < 2; ++e) { p[e] = have[e] ? expf(v[e] - bv) : 0.f; s += (double)p[e]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
#pragma unroll
    for (int e = 0; e < 2; ++e)
        if (lane + 64 * e < L) probs[(int64_t)r * L + lane + 64 * e] = (float)((double)p[e] / s);
    if (lane == 0) lang_token[r] = bi == 0x7fffffff ? -1 : bi;
}

__global__ __launch_bounds__(256) void gumbel_bits_kernel(uint32_t seed, uint32_t serial, int R, int V, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)R * V) return;
    out[i] = draw_bits(draw_key(seed, serial), (uint32_t)(i / V), (uint32_t)(i % V));
}

// x[r] = tok_emb[ids[r]] + pos_emb[position]
__global__ __launch_bounds__(256) void embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                   float* __restrict__ x, int R, int D4, int vocab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * D4) return;
    const int r = i / D4, d = i - r * D4;
    int id = ids[r];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const f32x4 a = reinterpret_cast<const f32x4*>(tok)[(int64_t)id * D4 + d], b = reinterpret_cast<const f32x4*>(pos)[d];
    reinterpret_cast<f32x4*>(x)[i] = a + b;
}

// x[r] = tok_emb[ids[r]] + pos_emb[ctl[r].position], and t[r] = that position for the self-attention.  A row whose position is
// outside [0, limit) is inactive: t[r] = -1, and so that the GEMMs it still passes through read defined values it embeds its clamped
// id at position 0 and its context row, which no attention block will write in the first layer, is zeroed.
__global__ __launch_bounds__(256) void embed_rows_kernel(const int32_t* __restrict__ ids, const hirest_whisper_row_ctl* __restrict__ ctl,
                                                        const float* __restrict__ tok, const float* __restrict__ pos, float* __restrict__ x,
                                                        float* __restrict__ ctx, int32_t* __restrict__ t, int R, int D4, int vocab, int limit) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * D4) return;
    const int r = i / D4, d = i - r * D4;
    const int p = ctl[r].position;
    const bool active = p >= 0 && p < limit;
    int id = ids[r];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const f32x4 a = reinterpret_cast<const f32x4*>(tok)[(int64_t)id * D4 + d];
    const f32x4 b = reinterpret_cast<const f32x4*>(pos)[(int64_t)(active ? p : 0) * D4 + d];
    reinterpret_cast<f32x4*>(x)[i] = a + b;
    if (!active) reinterpret_cast<f32x4*>(ctx)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (d == 0) t[r] = active ? p : -1;
}

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
inline int nchunks(int Tk) { return (Tk + XCH - 1) / XCH; }

struct Ws { size_t x, a, b, ln, qkv, ctx, mid, part, t, total; };
Ws plan(const hirest_whisper_decoder* d, int R, int Tk, bool rows = false) {
    Ws w; size_t off = 0;
    const size_t D = d->hidden;
    w.x = off; off += al((size_t)R * D * 4);
    w.a = off; off += al((size_t)R * D * 4);
    w.b = off; off += al((size_t)R * D * 4);
    w.ln = off; off += al((size_t)R * D * 4);
    w.qkv = off; off += al((size_t)R * 3 * D * 4);
    w.ctx = off; off += al((size_t)R * D * 4);
    w.mid = off; off += al((size_t)R * d->inter * 4);
    w.part = off; off += al((size_t)R * d->heads * nchunks(Tk) * XREC * 4);
    w.t = off; if (rows) off += al((size_t)R * 4);                // the rows' positions, behind everything the one-position step lays out
    w.total = off;
    return w;
}

#define CK(call) do { if (int e_ = (call)) return e_; } while (0)

// act(LayerNorm(X) W^T + bias): inside one GEMM where hirest_gemm_f32_ln has a form for the shape, else two calls — the same bits
int ln_gemm(const float* X, const float* g, const float* b, float* ln_scratch, const float* W, const float* bias, float* out, int R, int N,
            int K, int act, void* stream) {
    const float eps = 1e-5f;
    if (whisper_ln_gemm_fused(R, N, K))
        return hirest_gemm_f32_ln(X, K, nullptr, nullptr, nullptr, g, b, eps, nullptr, 0, W, K, bias, nullptr, 0, out, N, R, N, K, act, stream);
    CK(hirest_layernorm(X, K, nullptr, g, b, eps, ln_scratch, K, 1, R, K, stream));
    return hirest_gemm_f32(ln_scratch, K, W, K, bias, nullptr, 0, nullptr, 0, out, N, R, N, K, act, stream);
}

}  // namespace

extern "C" size_t hirest_attention_f32_cross_decode_workspace_bytes(int32_t R, int32_t H, int32_t Tk) {
    if (R <= 0 || H <= 0 || Tk <= 0) return 0;
    return (size_t)R * H * nchunks(Tk) * XREC * 4;
}

extern "C" int hirest_attention_f32_cross_decode(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int64_t window_stride,
                                                 int32_t n_windows, int32_t Tk, const int32_t* row_window, float* out, int64_t ldo, int32_t R,
                                                 int32_t H, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !kv || !row_window || !out || !workspace || R <= 0 || H <= 0 || Tk <= 0 || n_windows <= 0) return HIREST_E_BADARG;
    if (ldq % 4 != 0 || ldkv % 4 != 0 || window_stride % 4 != 0 || ldkv < 2 * (int64_t)H * 64 || ldq < (int64_t)H * 64 || ldo < (int64_t)H * 64 ||
        (n_windows > 1 && window_stride < (int64_t)Tk * ldkv))
        return HIREST_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(kv) & 15) != 0) return HIREST_E_SHAPE;
    if (workspace_bytes < hirest_attention_f32_cross_decode_workspace_bytes(R, H, Tk)) return HIREST_E_WORKSPACE;
    const int nc = nchunks(Tk);
    if ((int64_t)n_windows * H * nc > 0x7fffffffll) return HIREST_E_SHAPE;
    XDec p{q, ldq, kv, ldkv, window_stride, row_window, R, H, Tk, nc, n_windows, scale, static_cast<float*>(workspace), out, ldo};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cross_partial_kernel, dim3(n_windows * H * nc), dim3(256), 0, s, p);
    hipLaunchKernelGGL(cross_merge_kernel, dim3(R * H), dim3(64), 0, s, p);
    return hirest_launch_status();
}

extern "C" int hirest_whisper_step_tail(const float* logits, int64_t ldx, int32_t R, int32_t V, int32_t step, int32_t T_max,
                                        const hirest_whisper_tail_params* params, hirest_whisper_row_state* state, int32_t* next_ids,
                                        int32_t* tokens, float* logprobs, int32_t* done_host, void* stream) {
    if (!logits || !params || !state || !next_ids || !params->suppress_mask || R <= 0 || V <= 0 || step < 0) return HIREST_E_BADARG;
    const hirest_whisper_tail_params& c = *params;
    if (V % 4 != 0 || ldx % 4 != 0 || ldx < V || (reinterpret_cast<uintptr_t>(logits) & 15) != 0) return HIREST_E_SHAPE;
    if (logprobs && (reinterpret_cast<uintptr_t>(logprobs) & 15) != 0) return HIREST_E_SHAPE;
    if (c.n_vocab <= 0 || c.n_vocab > V || c.eot < 0 || c.eot >= c.n_vocab || c.no_speech >= c.n_vocab || c.blank >= c.n_vocab ||
        c.temperature < 0.f || c.sample_begin < 0)
        return HIREST_E_BADARG;
    if (c.timestamp_rules && (c.timestamp_begin <= c.eot || c.timestamp_begin > c.n_vocab || c.no_timestamps < 0 || c.no_timestamps >= c.n_vocab))
        return HIREST_E_BADARG;
    if (tokens && (T_max <= 0 || c.sample_begin + (int64_t)step >= T_max)) return HIREST_E_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(whisper_tail_kernel, dim3(R), dim3(1024), 0, s, logits, ldx, (int)V, (int)step, (int)T_max, c, state, next_ids, tokens, logprobs);
    if (done_host) hipLaunchKernelGGL(whisper_stamp_kernel, dim3(1), dim3(64), 0, s, state, (int)R, (int)step, done_host);
    return hirest_launch_status();
}

// call >= 0: the stamp carries `call`; count != null: it carries *count, which the stamp's launch advances.  One tail launch either way.
static int step_tail_rows(const float* logits, int64_t ldx, int32_t R, int32_t V, int32_t call, int32_t* count, int64_t ld_tokens,
                          const hirest_whisper_tail_params* params, hirest_whisper_row_ctl* ctl, hirest_whisper_row_state* state,
                          int32_t* next_ids, int32_t* tokens, float* logprobs, int32_t* done_host, void* stream) {
    if (!logits || !params || !ctl || !state || !next_ids || !tokens || !params->suppress_mask || R <= 0 || V <= 0 || call < 0 || ld_tokens <= 0)
        return HIREST_E_BADARG;
    const hirest_whisper_tail_params& c = *params;                // temperature, seed, serial and sample_begin: the rows' records replace them
    if (V % 4 != 0 || ldx % 4 != 0 || ldx < V || (reinterpret_cast<uintptr_t>(logits) & 15) != 0) return HIREST_E_SHAPE;
    if (logprobs && (reinterpret_cast<uintptr_t>(logprobs) & 15) != 0) return HIREST_E_SHAPE;
    if (c.n_vocab <= 0 || c.n_vocab > V || c.eot < 0 || c.eot >= c.n_vocab || c.no_speech >= c.n_vocab || c.blank >= c.n_vocab) return HIREST_E_BADARG;
    if (c.timestamp_rules && (c.timestamp_begin <= c.eot || c.timestamp_begin > c.n_vocab || c.no_timestamps < 0 || c.no_timestamps >= c.n_vocab))
        return HIREST_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(whisper_tail_rows_kernel, dim3(R), dim3(1024), 0, s, logits, ldx, (int)V, ld_tokens, c, ctl, state, next_ids, tokens, logprobs);
    if (count) hipLaunchKernelGGL(whisper_stamp_rows_counted_kernel, dim3(1), dim3(64), 0, s, ctl, (int)R, count, done_host);
    else if (done_host) hipLaunchKernelGGL(whisper_stamp_rows_kernel, dim3(1), dim3(64), 0, s, ctl, (int)R, (int)call, done_host);
    return hirest_launch_status();
}

extern "C" int hirest_whisper_step_tail_rows(const float* logits, int64_t ldx, int32_t R, int32_t V, int32_t call, int64_t ld_tokens,
                                             const hirest_whisper_tail_params* params, hirest_whisper_row_ctl* ctl,
                                             hirest_whisper_row_state* state, int32_t* next_ids, int32_t* tokens, float* logprobs,
                                             int32_t* done_host, void* stream) {
    return step_tail_rows(logits, ldx, R, V, call, nullptr, ld_tokens, params, ctl, state, next_ids, tokens, logprobs, done_host, stream);
}

extern "C" int hirest_whisper_step_tail_rows_counted(const float* logits, int64_t ldx, int32_t R, int32_t V, int32_t* count, int64_t ld_tokens,
                                                     const hirest_whisper_tail_params* params, hirest_whisper_row_ctl* ctl,
                                                     hirest_whisper_row_state* state, int32_t* next_ids, int32_t* tokens, float* logprobs,
                                                     int32_t* done_host, void* stream) {
    if (!count) return HIREST_E_BADARG;
    return step_tail_rows(logits, ldx, R, V, 0, count, ld_tokens, params, ctl, state, next_ids, tokens, logprobs, done_host, stream);
}

extern "C" int hirest_whisper_language_tail(const float* logits, int64_t ldx, int32_t R, int32_t V, const int32_t* language_ids, int32_t L,
                                            int32_t* lang_token, float* probs, void* stream) {
    if (!logits || !language_ids || !lang_token || !probs || R <= 0 || V <= 0) return HIREST_E_BADARG;
    if (L < 1 || L > 128 || ldx < V) return HIREST_E_SHAPE;
    hipLaunchKernelGGL(whisper_language_tail_kernel, dim3(R), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), logits, ldx, (int)V, language_ids,
                       (int)L, lang_token, probs);
    return hirest_launch_status();
}

extern "C" int hirest_whisper_gumbel_bits(uint32_t seed, uint32_t serial, int32_t R, int32_t V, uint32_t* out, void* stream) {
    if (!out || R <= 0 || V <= 0) return HIREST_E_BADARG;
    const int64_t n = (int64_t)R * V;
    hipLaunchKernelGGL(gumbel_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), seed, serial,
                       (int)R, (int)V, out);
    return hirest_launch_status();
}

extern "C" size_t hirest_whisper_step_workspace_bytes(const hirest_whisper_decoder* d, int32_t R, int32_t Tk) {
    if (!d || R <= 0 || Tk <= 0) return 0;
    return plan(d, R, Tk).total;
}

// One position of R rows.  ctl == null: every row at `position`.  Otherwise row r at ctl[r].position (rows outside [0, min(max_pos,
// T_max)) inactive): the embedding and the self-attention take the per-row form, every other call is the same one in the same order.
static int decode_step(const hirest_whisper_decoder* d, int32_t R, int32_t position, const hirest_whisper_row_ctl* ctl, const int32_t* ids,
                       float* const* self_k, float* const* self_v, int32_t T_max, const float* const* cross_kv, int32_t n_windows, int32_t Tk,
                const int32_t* row_window, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !d->layer || !ids || !self_k || !self_v || !cross_kv || !row_window || !logits || !workspace || R <= 0 || Tk <= 0 || n_windows <= 0)
        return HIREST_E_BADARG;
    if (!ctl && (position < 0 || position >= d->max_pos || position >= T_max)) return HIREST_E_BADARG;
    if (ctl && (T_max <= 0 || d->max_pos <= 0)) return HIREST_E_BADARG;
    const int D = d->hidden, H = d->heads, I = d->inter, Vp = d->vocab_padded;
    if (H <= 0 || D != H * 64 || D % 16 != 0 || I % 16 != 0 || Vp % 4 != 0) return HIREST_E_SHAPE;
    const Ws w = plan(d, R, Tk, ctl != nullptr);
    if (workspace_bytes < w.total) return HIREST_E_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    float* x = reinterpret_cast<float*>(base + w.x);
    float* a = reinterpret_cast<float*>(base + w.a);
    float* b = reinterpret_cast<float*>(base + w.b);
    float* ln = reinterpret_cast<float*>(base + w.ln);
    float* qkv = reinterpret_cast<float*>(base + w.qkv);
    float* ctx = reinterpret_cast<float*>(base + w.ctx);
    float* mid = reinterpret_cast<float*>(base + w.mid);
    void* part = base + w.part;
    int32_t* t_rows = reinterpret_cast<int32_t*>(base + w.t);
    const size_t part_bytes = w.t - w.part;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float scale = 0.125f;                                   // 64^-0.5: Whisper scales q and k by 64^-0.25 each
    if (ctl)
        hipLaunchKernelGGL(embed_rows_kernel, dim3((R * (D / 4) + 255) / 256), dim3(256), 0, s, ids, ctl, d->tok_emb, d->pos_emb, x, ctx, t_rows, (int)R,
                           D / 4, Vp, d->max_pos < T_max ? d->max_pos : T_max);
    else
        hipLaunchKernelGGL(embed_kernel, dim3((R * (D / 4) + 255) / 256), dim3(256), 0, s, ids, d->tok_emb, d->pos_emb + (int64_t)position * D, x,
                           (int)R, D / 4, Vp);
    for (int i = 0; i < d->layers; ++i) {
        const hirest_whisper_layer& L = d->layer[i];
        CK(ln_gemm(x, L.attn_ln_g, L.attn_ln_b, ln, L.qkv_w, L.qkv_b, qkv, R, 3 * D, D, 0, stream));
        if (ctl)
            CK(hirest_attention_f32_decode_inplace_rows(qkv, 3 * D, self_k[i], self_v[i], D, (int64_t)T_max * D, t_rows, T_max, qkv + D, qkv + 2 * D,
                                                        3 * D, ctx, R, H, scale, 0.f, 0.f, stream));
        else
            CK(hirest_attention_f32_decode_inplace(qkv, 3 * D, self_k[i], self_v[i], D, (int64_t)T_max * D, position, T_max, qkv + D, qkv + 2 * D,
                                                   3 * D, ctx, R, H, scale, 0.f, 0.f, stream));
        CK(hirest_gemm_f32(ctx, D, L.so_w, D, L.so_b, x, D, nullptr, 0, a, D, R, D, D, 0, stream));
        CK(ln_gemm(a, L.cross_ln_g, L.cross_ln_b, ln, L.cq_w, L.cq_b, qkv, R, D, D, 0, stream));
        CK(hirest_attention_f32_cross_decode(qkv, D, cross_kv[i], 2 * D, (int64_t)Tk * 2 * D, n_windows, Tk, row_window, ctx, D, R, H, scale, part,
                                             part_bytes, stream));
        CK(hirest_gemm_f32(ctx, D, L.co_w, D, L.co_b, a, D, nullptr, 0, b, D, R, D, D, 0, stream));
        CK(ln_gemm(b, L.mlp_ln_g, L.mlp_ln_b, ln, L.fc1_w, L.fc1_b, mid, R, I, D, 1, stream));
        CK(hirest_gemm_f32(mid, I, L.fc2_w, I, L.fc2_b, b, D, nullptr, 0, x, D, R, D, I, 0, stream));
    }
    CK(ln_gemm(x, d->ln_g, d->ln_b, ln, d->tok_emb, d->lm_b, logits, R, Vp, D, 0, stream));
    return hirest_launch_status();
}

extern "C" int hirest_whisper_decode_step(const hirest_whisper_decoder* d, int32_t R, int32_t position, const int32_t* ids,
                                          float* const* self_k, float* const* self_v, int32_t T_max, const float* const* cross_kv,
                                          int32_t n_windows, int32_t Tk, const int32_t* row_window, float* logits, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return decode_step(d, R, position, nullptr, ids, self_k, self_v, T_max, cross_kv, n_windows, Tk, row_window, logits, workspace, workspace_bytes,
                       stream);
}

extern "C" size_t hirest_whisper_step_rows_workspace_bytes(const hirest_whisper_decoder* d, int32_t R, int32_t Tk) {
    if (!d || R <= 0 || Tk <= 0) return 0;
    return plan(d, R, Tk, true).total;
}

extern "C" int hirest_whisper_decode_step_rows(const hirest_whisper_decoder* d, int32_t R, const hirest_whisper_row_ctl* ctl, const int32_t* ids,
                                               float* const* self_k, float* const* self_v, int32_t T_max, const float* const* cross_kv,
                                               int32_t n_windows, int32_t Tk, const int32_t* row_window, float* logits, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!ctl) return HIREST_E_BADARG;
    return decode_step(d, R, 0, ctl, ids, self_k, self_v, T_max, cross_kv, n_windows, Tk, row_window, logits, workspace, workspace_bytes, stream);
}
