// What the Whisper decoder's C files share (whisper_dec.hip: the decoding step; whisper_prefill.hip: the prompt prefill).
#pragma once

// Whether act(LayerNorm(X) W^T + bias) for R rows, N columns and depth K runs inside one GEMM (hirest_gemm_f32_ln has a form for the
// shape) or as hirest_layernorm + hirest_gemm_f32 — the same bits either way.  The step and the prefill must route alike, and so
// must whisper.py's _ln_linear, whose condition is this one.
static inline bool whisper_ln_gemm_fused(int R, int N, int K) {
    return R <= 256 && K % 256 == 0 && K <= 1024 && (N < 8192 || (K == 768 && R <= 32));
}
