// Whisper audio encoder, split-operand precision ("bf16x3", include/hirest_hip.h: hirest_whisper_encoder_x3): the pre-LN blocks of
// whisper/model.py's AudioEncoder (ResidualAttentionBlock without cross attention: x += attn(attn_ln(x)); x += mlp(mlp_ln(x)); ln_post after
// the last one) with the four weight products of every block and both attention products on the bf16 matrix pipe — three MFMAs per product on
// bf16 hi + lo splits of both fp32 operands, fp32 accumulation.  The residual stream, the LayerNorm statistics and the softmax stay fp32.  The
// stem (conv1, conv2, GELU, positional embedding) is not here: the caller passes its exact-fp32 output.
//
// This file holds no kernel: one C call issues, per block, seven launches of kernels the towers and the joint model already run —
//   hirest_layernorm_split2 -> qkv (x3, fp32 out) -> hirest_attention_x3_qkv_split2 -> out projection (x3, += residual)
//   -> hirest_layernorm_split2 -> fc1 (x3, GELU + split in the epilogue) -> fc2 (x3, += residual)
// — instead of the 7 host-language calls per block of the fp32 path.
//
// Every product takes the 128 x 128 split-operand kernel (HIREST_GEMM_X3_T128) at every row count, without its split-K form: gemm_t128x3 and
// gemm_pp256x3 add a row's products in different orders (two 16-deep K groups per step against one 32-deep MFMA), and a split-K slice count
// depends on the number of tiles, so any choice of family or slicing by M would make a window's bits depend on how many windows share the call.
// One family, one K order: a clip encoded alone equals its rows of a batched call (tests/test_gpu_whisper_x3.py).
#include "common.h"
#include "profile.h"

namespace {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
#define CHECK(expr) do { int _e = (expr); if (_e != 0) return _e; } while (0)

// The hirest_gemm_bf16 call of product `which` (HIREST_WHISPER_X3_QKV ...) of a block over M rows, without its pointers: the one place that
// decides shape, epilogue and flags — the forward fills the pointers in, hirest_whisper_encoder_x3_gemm_args hands it out as it is.
hirest_gemm_args product(const hirest_whisper_encoder_x3* e, int M, int which) {
    const int D = e->width, F = e->ffn;
    const bool gelu_pass = (e->flags & HIREST_WHISPER_X3_GELU_PASS) != 0;
    hirest_gemm_args a;
    a.struct_size = sizeof(a);
    a.A = nullptr; a.W = nullptr; a.bias = nullptr; a.out = nullptr; a.pos = nullptr; a.patches_per_frame = 0; a.aux0 = a.aux1 = nullptr;
    a.M = M;
    a.flags = HIREST_GEMM_X3 | ((e->flags & HIREST_WHISPER_X3_AUTO_TILES) ? 0 : HIREST_GEMM_X3_T128);
    int N, K, epi; int64_t ldo;
    switch (which) {
        case HIREST_WHISPER_X3_QKV: N = 3 * D; K = D; epi = HIREST_EPI_BIAS_F32; ldo = N; break;
        case HIREST_WHISPER_X3_OUT: N = D; K = D; epi = HIREST_EPI_BIAS_RESID_F32; ldo = N; break;
        case HIREST_WHISPER_X3_FC1: N = F; K = D; epi = gelu_pass ? HIREST_EPI_BIAS_F32 : HIREST_EPI_BIAS_GELU_SPLIT2; ldo = gelu_pass ? N : 2 * N; break;
        default: N = D; K = F; epi = HIREST_EPI_BIAS_RESID_F32; ldo = N; break;       // HIREST_WHISPER_X3_FC2
    }
    a.N = N; a.K = 2 * K; a.lda = a.ldw = 2 * K; a.ldo = ldo; a.epilogue = epi;
    return a;
}

int gemm_x3(hirest_gemm_args a, const hirest_bf16* A2, const hirest_bf16* W2, const float* bias, void* out, void* stream) {
    a.A = A2; a.W = W2; a.bias = bias; a.out = out;
    return hirest_gemm_bf16(&a, stream);
}

struct RegionsW { size_t x, a2, big, h2, total; };
RegionsW plan(int64_t M, int D, int F) {
    RegionsW r; size_t off = 0;
    const int wide = 3 * D > F ? 3 * D : F;
    r.x = off; off += align256((size_t)M * D * 4);                   // the fp32 residual stream
    r.a2 = off; off += align256((size_t)M * 2 * D * 2);               // split A operand of qkv / out / fc1
    r.big = off; off += align256((size_t)M * wide * 4);               // q | k | v rows (and fc1's fp32 output under HIREST_WHISPER_X3_GELU_PASS)
    r.h2 = off; off += align256((size_t)M * 2 * F * 2);               // split hidden activation: fc2's A operand
    r.total = off;
    return r;
}

bool shape_ok(const hirest_whisper_encoder_x3* e) {
    if (e->layers <= 0 || e->heads <= 0 || e->width <= 0 || e->ffn <= 0 || e->ctx <= 0) return false;
    if (e->width % e->heads != 0 || e->width % 32 != 0 || e->ffn % 32 != 0 || e->width > 2048) return false;
    const int dh = e->width / e->heads;
    return dh % 4 == 0 && dh <= 96;                                   // hirest_attention_x3_*'s head widths
}

}  // namespace

extern "C" size_t hirest_whisper_encoder_x3_workspace_bytes(const hirest_whisper_encoder_x3* e, int32_t B) {
    if (!e || e->struct_size != sizeof(*e) || B <= 0 || !shape_ok(e)) return 0;
    return plan((int64_t)B * e->ctx, e->width, e->ffn).total;
}

extern "C" int hirest_whisper_encoder_x3_gemm_args(const hirest_whisper_encoder_x3* e, int32_t B, int32_t which, hirest_gemm_args* out) {
    if (!e || e->struct_size != sizeof(*e) || !out || B <= 0 || which < HIREST_WHISPER_X3_QKV || which > HIREST_WHISPER_X3_FC2) return HIREST_E_BADARG;
    if (!shape_ok(e) || (int64_t)B * e->ctx > 0x7fffffff) return HIREST_E_SHAPE;
    *out = product(e, B * e->ctx, which);
    return 0;
}

extern "C" int hirest_whisper_encoder_x3_forward(const hirest_whisper_encoder_x3* e, const float* x_in, int32_t B, float* out, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
    if (!e || e->struct_size != sizeof(*e) || !x_in || !out || !workspace || B <= 0 || !e->layer || !e->ln_post_g || !e->ln_post_b)
        return HIREST_E_BADARG;
    if (e->flags & ~(HIREST_WHISPER_X3_GELU_PASS | HIREST_WHISPER_X3_AUTO_TILES)) return HIREST_E_BADARG;
    if (!shape_ok(e)) return HIREST_E_SHAPE;
    const int64_t M64 = (int64_t)B * e->ctx;
    if (M64 > 0x7fffffff) return HIREST_E_SHAPE;
    const int M = (int)M64, D = e->width, F = e->ffn, T = e->ctx, H = e->heads, dh = D / H;
    const RegionsW r = plan(M64, D, F);
    if (workspace_bytes < r.total) return HIREST_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(x_in) | reinterpret_cast<uintptr_t>(out)) & 15) return HIREST_E_SHAPE;
    char* ws = reinterpret_cast<char*>(workspace);
    float* x = reinterpret_cast<float*>(ws + r.x);
    hirest_bf16* a2 = reinterpret_cast<hirest_bf16*>(ws + r.a2);
    float* big = reinterpret_cast<float*>(ws + r.big);
    hirest_bf16* h2 = reinterpret_cast<hirest_bf16*>(ws + r.h2);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)dh);
    const bool gelu_pass = (e->flags & HIREST_WHISPER_X3_GELU_PASS) != 0;     // (measurement switch of the descriptor: the shipped path is flags == 0)
    const hirest_gemm_args qkv = product(e, M, HIREST_WHISPER_X3_QKV), proj = product(e, M, HIREST_WHISPER_X3_OUT),
                           fc1 = product(e, M, HIREST_WHISPER_X3_FC1), fc2 = product(e, M, HIREST_WHISPER_X3_FC2);
    // the residual epilogues add in place: the stem's rows are the caller's, the stream lives in the workspace
    if (hipError_t err = hipMemcpyAsync(x, x_in, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s)) return (int)err;
    for (int l = 0; l < e->layers; ++l) {
        const hirest_whisper_layer_x3& w = e->layer[l];
        if (!w.attn_ln_g || !w.attn_ln_b || !w.qkv_w2 || !w.qkv_b || !w.out_w2 || !w.out_b || !w.mlp_ln_g || !w.mlp_ln_b || !w.fc1_w2 || !w.fc1_b ||
            !w.fc2_w2 || !w.fc2_b)
            return HIREST_E_BADARG;
        // (profile records of the non-GEMM kernels, as the bf16x3 tower tags them: kind LAYERNORM tag 10 LayerNorm + split, 12 GELU + split;
        //  kind ATTENTION tag 2)
        { HirestProfScope pr(HIREST_PROF_LAYERNORM, 10, M, D, 0, s);
          CHECK(hirest_layernorm_split2(x, D, w.attn_ln_g, w.attn_ln_b, e->ln_eps, a2, 2 * D, M, D, stream)); }
        CHECK(gemm_x3(qkv, a2, w.qkv_w2, w.qkv_b, big, stream));
        { HirestProfScope pr(HIREST_PROF_ATTENTION, 2, (int64_t)B * H, T, dh, s);       // writes the out projection's split operand itself
          CHECK(hirest_attention_x3_qkv_split2(big, 3 * (int64_t)D, big + D, big + 2 * D, 3 * (int64_t)D, a2, B, T, T, H, dh, scale, stream)); }
        CHECK(gemm_x3(proj, a2, w.out_w2, w.out_b, x, stream));
        { HirestProfScope pr(HIREST_PROF_LAYERNORM, 10, M, D, 0, s);
          CHECK(hirest_layernorm_split2(x, D, w.mlp_ln_g, w.mlp_ln_b, e->ln_eps, a2, 2 * D, M, D, stream)); }
        if (!gelu_pass) {                                             // the hidden activation never exists in fp32
            CHECK(gemm_x3(fc1, a2, w.fc1_w2, w.fc1_b, h2, stream));
        } else {
            CHECK(gemm_x3(fc1, a2, w.fc1_w2, w.fc1_b, big, stream));
            HirestProfScope pr(HIREST_PROF_LAYERNORM, 12, M, F, 0, s);
            CHECK(hirest_split2_bf16(big, F, h2, 2 * F, M, F, 1, stream));
        }
        CHECK(gemm_x3(fc2, h2, w.fc2_w2, w.fc2_b, x, stream));
    }
    CHECK(hirest_layernorm(x, D, nullptr, e->ln_post_g, e->ln_post_b, e->ln_eps, out, D, 1, M, D, stream));
    return 0;
}
