"""CPU-side checks: the C-ABI library builds/loads and exports every symbol the header declares
(no compute calls without a GPU), and the host layer mirrors the reference interface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_header_symbols_all_exported(lib):
    from hirest_amd import _lib
    hdr = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hirest_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 18
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/hirest_hip.h but not exported"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert lib.hirest_abi_version() == 4 == _lib.ABI_VERSION
    assert b"gfx950" in lib.hirest_build_info()


def test_argument_errors_without_gpu(lib):
    from hirest_amd import _lib
    a = _lib.GemmArgs()  # all-NULL
    assert lib.hirest_gemm_bf16(ctypes.byref(a), None) == -1
    # a binding built against another struct layout (ABI 2 had no struct_size / flags) is rejected before any member
    # behind its end is read: non-NULL operands, valid shape, wrong struct_size -> BADARG, never a launch
    b = _lib.GemmArgs(ctypes.sizeof(_lib.GemmArgs) - 8, 1 << 20, 64, 1 << 21, 64, None, 1 << 22, 64, 64, 64, 64, 0)
    assert lib.hirest_gemm_bf16(ctypes.byref(b), None) == -1
    assert _lib.GemmArgs.make().struct_size == ctypes.sizeof(_lib.GemmArgs) == 120
    assert lib.hirest_layernorm(None, 0, None, None, None, 0.0, None, 0, 0, 0, 0, None) == -1
    assert lib.hirest_attention_bf16(None, None, 1, 1, 1, 64, 1.0, 0, None) == -1
    assert lib.hirest_vision_workspace_bytes(None, 4) == 0
    # round-2 entry points: captioning step, beam bookkeeping, ragged BERT batch, fp32 GEMM selector
    d = _lib.CaptionDecoder(2, 12, 768, 3072, 30528, 512)
    al = lambda v: (v + 255) // 256 * 256
    assert lib.hirest_caption_step_workspace_bytes(ctypes.byref(d), 25) == \
        5 * al(25 * 768 * 4) + al(25 * 3 * 768 * 4) - al(25 * 768 * 4) + al(25 * 3072 * 4) + al(25 * 30528 * 4) + al(25 * 4) + al(25 * 1908 * 4)
    assert lib.hirest_caption_step_workspace_bytes(None, 25) == 0
    assert lib.hirest_caption_decode_step(ctypes.byref(d), 25, 0, None, None, None, None, None, 20, None, None, None, 0, None) == -1
    assert lib.hirest_beam_advance(None, None, 5, 5, 30528, 0, 48, 102, None, None, None, None, None, None, None, None, None) == -1
    assert lib.hirest_attention_f32_varlen(None, None, None, 1, 1, 12, 64, 0.125, 0.0, None) == -1
    assert lib.hirest_pool_l2norm_varlen(None, None, None, 1, 384, None) == -1
    assert lib.hirest_embedding_pos_fwd_f32(None, None, None, None, None, 1, 384, None) == -1
    assert lib.hirest_gemm_f32_select_kernel(3) == -1 and lib.hirest_gemm_f32_select_kernel(0) == 0
    # round 3: the step-captioning decode kernels
    assert lib.hirest_caption_select(2) == -1 and lib.hirest_caption_select(0) == 0
    assert lib.hirest_caption_decode_logits(ctypes.byref(d), 25, 0, None, None, None, None, None, 20, None, None, 0, None) == -1
    assert lib.hirest_caption_beam_tail_workspace_bytes(5, 5, 30528) == 25 * 8 * 5 * 8 + 25 * 17 * 4     # candidates (score, index) + row statistics
    assert lib.hirest_caption_beam_tail_workspace_bytes(0, 5, 30528) == 0
    assert lib.hirest_caption_beam_tail(None, 30528, None, 5, 5, 30528, 0, 48, 102, None, None, None, None, None, None, None, None, None, None, 0,
                                        None) == -1
    assert lib.hirest_gemm_f32_ln(None, 768, None, None, None, None, None, 1e-12, None, 0, None, 768, None, None, 0, None, 768, 25, 768, 768, 0,
                                  None) == -1
    assert lib.hirest_attention_f32_decode(None, 768, None, None, 768, None, 0, None, None, 0, None, None, None, 25, 12, 0.125, 0.0, 0.0, None) == -1
    assert lib.hirest_caption_beam_step(ctypes.byref(d), 5, 5, 0, None, None, None, None, None, 20, None, None, 48, 102, None, None, None, None,
                                        None, None, None, 0, None, 0, None) == -1
    assert lib.hirest_gemm_f32_ln_colmax(None, 768, None, None, 1e-12, None, 768, None, None, 30528, None, 25, 30528, 768, None) == -1
    assert lib.hirest_gemm_f32_workspace_bytes(1500, 768, 3072) == 4 * 1500 * 768 * 4       # 288 tiles: split over the four K quarters
    assert lib.hirest_gemm_f32_workspace_bytes(1500, 3072, 768) == 0 and lib.hirest_gemm_f32_workspace_bytes(25, 768, 3072) == 0
    assert lib.hirest_gemm_f32_ws(None, 768, None, 768, None, None, 0, None, 0, None, 768, 1500, 768, 3072, 0, None, 0, None) == -1
    assert lib.hirest_gemm_f32_layouts(None, 768, 1, None, 768, 1, None, None, 0, None, 768, 768, 768, 1500, 0, None, 0, None) == -1
    assert lib.hirest_gemm_f32_layouts_workspace_bytes(768, 768, 1500) == 4 * 768 * 768 * 4 and lib.hirest_gemm_f32_layouts_workspace_bytes(3072, 3072, 1500) == 0
    assert lib.hirest_joint_time_grid_f32(None, 5, 300, None, None) == -1
    from hirest_amd._lib import ColsumItem, COLSUM_GROUP_MAX
    assert ctypes.sizeof(ColsumItem) == 56 and COLSUM_GROUP_MAX == 40       # hirest_colsum_item / HIREST_COLSUM_GROUP_MAX
    assert lib.hirest_weighted_colsum_grouped_f32(None, 3, None) == -1
    assert lib.hirest_weighted_colsum_grouped_f32((ColsumItem * 2)(), 2, None) == -1     # NULL matrices: refused before any launch
    # round 6: the joint model's bf16x3 pieces, the C-issued training step, the captioning read-out
    assert lib.hirest_layernorm_f32_split2(None, 768, None, 0, None, None, 1e-12, None, 768, None, 1536, 5, 768, None) == -1
    assert lib.hirest_split2_transposed_bf16(None, 768, None, 1536, 768, 768, None) == -1
    assert ctypes.sizeof(_lib.SplitItem) == 48
    assert lib.hirest_split2_grouped_bf16(None, 2, None) == -1 and lib.hirest_split2_grouped_bf16((_lib.SplitItem * 2)(), 2, None) == -1
    assert lib.hirest_beam_backtrack(None, None, None, None, 5, 5, 48, None, None) == -1
    tb = _lib.TrainBlock()
    assert lib.hirest_train_block_forward_scratch_bytes(ctypes.byref(tb)) == 0                 # struct_size 0: another layout
    tb.struct_size = ctypes.sizeof(_lib.TrainBlock)
    tb.B, tb.T, tb.heads, tb.width, tb.mlp = 5, 300, 12, 768, 3072
    al64 = lambda n: (n + 63) // 64 * 64
    R = 1500
    assert lib.hirest_train_block_forward_scratch_bytes(ctypes.byref(tb)) == 4 * al64(R * 768)
    assert lib.hirest_train_block_backward_scratch_bytes(ctypes.byref(tb)) == \
        4 * (8 * al64(R * 768) + 2 * al64(R * 3072) + al64(5 * 12 * 300 * 300) + al64(R * 2304))
    tb.precision = 1
    assert lib.hirest_train_block_forward_scratch_bytes(ctypes.byref(tb)) > 4 * al64(R * 768)
    tb.precision = 2
    assert lib.hirest_train_block_forward_scratch_bytes(ctypes.byref(tb)) == 0                 # unknown precision
    tb.precision = 0
    assert lib.hirest_train_block_forward(ctypes.byref(tb), None, 0, None) == -1               # no scratch: refused before any launch
    tg = _lib.TrainBlockGrads()
    assert lib.hirest_train_block_backward(ctypes.byref(tb), ctypes.byref(tg), None) == -1     # struct_size 0
    tf = _lib.TrainFusionBwd()
    assert lib.hirest_train_fusion_backward_scratch_bytes(ctypes.byref(tf)) == 0 and lib.hirest_train_fusion_backward(ctypes.byref(tf), None) == -1
    tf.struct_size = ctypes.sizeof(_lib.TrainFusionBwd)
    tf.B, tf.T, tf.E, tf.W, tf.vis_dim, tf.text_dim, tf.asr_dim, tf.max_pos = 5, 300, 512, 768, 1024, 1024, 384, 2048
    assert lib.hirest_train_fusion_backward_scratch_bytes(ctypes.byref(tf)) > 0
    assert lib.hirest_train_fusion_backward(ctypes.byref(tf), None) == -1                      # no dx / scratch
    tf.T = 4096
    assert lib.hirest_train_fusion_backward_scratch_bytes(ctypes.byref(tf)) == 0               # longer than the position table


def test_train_entry_points_refuse_bad_arguments_without_gpu(lib):
    """Every entry point of csrc/train.hip checks its arguments before any launch: NULL pointers and non-positive sizes give
    HIREST_E_BADARG (-1), an unsupported head size or dropout rate HIREST_E_SHAPE (-2).  The placeholder pointers X are never
    dereferenced: each call below is refused by its checks alone."""
    X = 1 << 20
    BAD, SHAPE = -1, -2
    # transpose_pad(in, ld, R, C, out, Rp): Rp < R
    assert lib.hirest_transpose_pad_f32(None, 8, 2, 2, X, 2, None) == BAD
    assert lib.hirest_transpose_pad_f32(X, 8, 2, 2, None, 2, None) == BAD
    assert lib.hirest_transpose_pad_f32(X, 8, 0, 2, X, 2, None) == BAD
    assert lib.hirest_transpose_pad_f32(X, 8, 2, 0, X, 2, None) == BAD
    assert lib.hirest_transpose_pad_f32(X, 8, 4, 2, X, 3, None) == BAD
    # weighted_colsum(x, ldx, w, sel, value, R, C, out)
    assert lib.hirest_weighted_colsum_f32(None, 8, None, None, 0, 2, 2, X, None) == BAD
    assert lib.hirest_weighted_colsum_f32(X, 8, None, None, 0, 2, 2, None, None) == BAD
    assert lib.hirest_weighted_colsum_f32(X, 8, None, None, 0, 0, 2, X, None) == BAD
    assert lib.hirest_weighted_colsum_f32(X, 8, None, None, 0, 2, -1, X, None) == BAD
    # scale_by_device_scalar(x, scalar, n)
    assert lib.hirest_scale_by_device_scalar_f32(None, X, 4, None) == BAD
    assert lib.hirest_scale_by_device_scalar_f32(X, None, 4, None) == BAD
    assert lib.hirest_scale_by_device_scalar_f32(X, X, 0, None) == BAD
    # act(pre, y, n, act): 0..2 forward; act_bwd(pre, dy, dx, n, act): 0..3
    assert lib.hirest_act_f32(None, X, 4, 1, None) == BAD and lib.hirest_act_f32(X, None, 4, 1, None) == BAD
    assert lib.hirest_act_f32(X, X, 0, 1, None) == BAD
    assert lib.hirest_act_f32(X, X, 4, -1, None) == BAD and lib.hirest_act_f32(X, X, 4, 3, None) == BAD
    assert lib.hirest_act_bwd_f32(None, X, X, 4, 1, None) == BAD and lib.hirest_act_bwd_f32(X, None, X, 4, 1, None) == BAD
    assert lib.hirest_act_bwd_f32(X, X, None, 4, 1, None) == BAD and lib.hirest_act_bwd_f32(X, X, X, -3, 1, None) == BAD
    assert lib.hirest_act_bwd_f32(X, X, X, 4, -1, None) == BAD and lib.hirest_act_bwd_f32(X, X, X, 4, 4, None) == BAD
    # dropout_add(x, resid, y, n, p, seed): 0 <= p < 1
    assert lib.hirest_dropout_add_f32(None, None, X, 4, 0.1, 0, None) == BAD
    assert lib.hirest_dropout_add_f32(X, None, None, 4, 0.1, 0, None) == BAD
    assert lib.hirest_dropout_add_f32(X, None, X, 0, 0.1, 0, None) == BAD
    for p in (1.0, 1.5, -0.1, float("nan")):
        assert lib.hirest_dropout_add_f32(X, None, X, 4, p, 0, None) == BAD, p
    # layernorm_bwd(x, dy, gamma, eps, dx, dyxhat, R, D)
    for i in range(5):
        ptrs = [X] * 5
        ptrs[i] = None
        assert lib.hirest_layernorm_bwd_f32(ptrs[0], ptrs[1], ptrs[2], 1e-12, ptrs[3], ptrs[4], 4, 768, None) == BAD, i
    assert lib.hirest_layernorm_bwd_f32(X, X, X, 1e-12, X, X, 0, 768, None) == BAD
    assert lib.hirest_layernorm_bwd_f32(X, X, X, 1e-12, X, X, 4, 0, None) == BAD
    # attention, general form: fwd(q, ldq, k, v, ldkv, mask, P, ctx, ldctx, B, Tq, Tk, H, dh, scale, add_const, drop, seed)
    fwd = lambda q, k, v, P, c, B, Tq, Tk, H, dh, drop: lib.hirest_attention_train_fwd_qkv_f32(
        q, 768, k, v, 1536, None, P, c, 768, B, Tq, Tk, H, dh, 0.125, 0.0, drop, 0, None)
    for i in range(5):
        ptrs = [X] * 5
        ptrs[i] = None
        assert fwd(*ptrs, 2, 3, 5, 12, 64, 0.1) == BAD, i
    for dims in ((0, 3, 5, 12), (2, 0, 5, 12), (2, 3, 0, 12), (2, 3, 5, 0)):
        assert fwd(X, X, X, X, X, *dims, 64, 0.1) == BAD, dims
    assert fwd(X, X, X, X, X, 2, 3, 5, 12, 32, 0.1) == SHAPE and fwd(X, X, X, X, X, 2, 3, 5, 12, 128, 0.0) == SHAPE
    assert fwd(X, X, X, X, X, 2, 3, 5, 12, 64, 1.0) == SHAPE and fwd(X, X, X, X, X, 2, 3, 5, 12, 64, -0.5) == SHAPE
    # bwd(q, ldq, k, v, ldkv, P, dctx, ldctx, dS, dq, lddq, dk, dv, lddkv, B, Tq, Tk, H, dh, scale, drop, seed)
    bwd = lambda ptrs, B, Tq, Tk, H, dh, drop: lib.hirest_attention_train_bwd_qkv_f32(
        ptrs[0], 768, ptrs[1], ptrs[2], 1536, ptrs[3], ptrs[4], 768, ptrs[5], ptrs[6], 768, ptrs[7], ptrs[8], 1536, B, Tq, Tk, H, dh, 0.125,
        drop, 0, None)
    for i in range(9):
        ptrs = [X] * 9
        ptrs[i] = None
        assert bwd(ptrs, 2, 3, 5, 12, 64, 0.1) == BAD, i
    for dims in ((0, 3, 5, 12), (2, -1, 5, 12), (2, 3, 0, 12), (2, 3, 5, 0)):
        assert bwd([X] * 9, *dims, 64, 0.1) == BAD, dims
    assert bwd([X] * 9, 2, 3, 5, 12, 80, 0.1) == SHAPE and bwd([X] * 9, 2, 3, 5, 12, 64, 1.0) == SHAPE
    # packed self-attention forms
    assert lib.hirest_attention_train_fwd_f32(None, X, X, 2, 5, 12, 64, 0.125, 0.0, 0.1, 0, None) == BAD
    assert lib.hirest_attention_train_fwd_f32(X, X, X, 2, 5, 12, 96, 0.125, 0.0, 0.1, 0, None) == SHAPE
    assert lib.hirest_attention_train_fwd_f32(X, X, X, 2, 5, 12, 64, 0.125, 0.0, 1.0, 0, None) == SHAPE
    assert lib.hirest_attention_train_bwd_f32(X, X, X, X, None, 2, 5, 12, 64, 0.125, 0.1, 0, None) == BAD
    assert lib.hirest_attention_train_bwd_f32(None, X, X, X, X, 2, 5, 12, 64, 0.125, 0.1, 0, None) == BAD
    assert lib.hirest_attention_train_bwd_f32(X, X, X, X, X, 2, 5, 12, 16, 0.125, 0.1, 0, None) == SHAPE
    assert lib.hirest_attention_train_select(2) == BAD and lib.hirest_attention_train_select(-1) == BAD
    # gemm_f32_strided(A, sam, sak, B, sbn, sbk, C, ldc, M, N, K, alpha): one stride of each pair must be 1
    gs = lambda A, sam, sak, B, sbn, sbk, C, M, N, K: lib.hirest_gemm_f32_strided(A, sam, sak, B, sbn, sbk, C, 64, M, N, K, 1.0, None)
    assert gs(None, 64, 1, X, 64, 1, X, 8, 8, 8) == BAD and gs(X, 64, 1, None, 64, 1, X, 8, 8, 8) == BAD
    assert gs(X, 64, 1, X, 64, 1, None, 8, 8, 8) == BAD
    for dims in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-8, 8, 8)):
        assert gs(X, 64, 1, X, 64, 1, X, *dims) == BAD, dims
    assert gs(X, 64, 2, X, 64, 1, X, 8, 8, 8) == SHAPE and gs(X, 64, 1, X, 3, 5, X, 8, 8, 8) == SHAPE
    # embeddings
    assert lib.hirest_embedding_fwd_f32(None, X, X, X, 4, 2, 8, None) == BAD and lib.hirest_embedding_fwd_f32(X, None, X, X, 4, 2, 8, None) == BAD
    assert lib.hirest_embedding_fwd_f32(X, X, None, X, 4, 2, 8, None) == BAD and lib.hirest_embedding_fwd_f32(X, X, X, None, 4, 2, 8, None) == BAD
    for dims in ((0, 2, 8), (4, 0, 8), (4, 2, 0)):
        assert lib.hirest_embedding_fwd_f32(X, X, X, X, *dims, None) == BAD, dims
    assert lib.hirest_embedding_pos_fwd_f32(X, None, X, X, X, 4, 8, None) == BAD
    assert lib.hirest_embedding_pos_fwd_f32(X, X, X, X, X, 0, 8, None) == BAD and lib.hirest_embedding_pos_fwd_f32(X, X, X, X, X, 4, 0, None) == BAD
    assert lib.hirest_embedding_bwd_f32(None, X, X, 4, 8, None) == BAD and lib.hirest_embedding_bwd_f32(X, X, None, 4, 8, None) == BAD
    assert lib.hirest_embedding_bwd_f32(X, X, X, 0, 8, None) == BAD and lib.hirest_embedding_bwd_f32(X, X, X, 4, 0, None) == BAD
    # ce_rows(logits, ld, target, R, V, weight, n_valid, loss, dlogits): ld >= V
    ce = lambda lg, ld, tg, R, V, ls, dl: lib.hirest_ce_rows_f32(lg, ld, tg, R, V, 1.0, 2, ls, dl, None)
    assert ce(X, 10, X, 2, 11, X, X) == BAD
    assert ce(None, 16, X, 2, 11, X, X) == BAD and ce(X, 16, None, 2, 11, X, X) == BAD
    assert ce(X, 16, X, 2, 11, None, X) == BAD and ce(X, 16, X, 2, 11, X, None) == BAD
    assert ce(X, 16, X, 0, 11, X, X) == BAD and ce(X, 16, X, 2, 0, X, X) == BAD
    # masked losses (logits, target|mask, mask|target, B, T, weight, loss, dlogits)
    for fn in (lib.hirest_bce_masked_f32, lib.hirest_ce_masked_f32):
        for i in range(5):
            ptrs = [X] * 5
            ptrs[i] = None
            assert fn(ptrs[0], ptrs[1], ptrs[2], 2, 5, 1.0, ptrs[3], ptrs[4], None) == BAD, (fn, i)
        assert fn(X, X, X, 0, 5, 1.0, X, X, None) == BAD and fn(X, X, X, 2, 0, 1.0, X, X, None) == BAD
    # fusion backward pieces
    for i in range(5):
        ptrs = [X] * 5
        ptrs[i] = None
        assert lib.hirest_joint_base_bwd_f32(*ptrs, 2, 5, 8, None) == BAD, i
    for dims in ((0, 5, 8), (2, 0, 8), (2, 5, 0)):
        assert lib.hirest_joint_base_bwd_f32(X, X, X, X, X, *dims, None) == BAD, dims
    assert lib.hirest_l2norm_bwd_f32(None, X, X, 2, 8, None) == BAD and lib.hirest_l2norm_bwd_f32(X, None, X, 2, 8, None) == BAD
    assert lib.hirest_l2norm_bwd_f32(X, X, None, 2, 8, None) == BAD
    assert lib.hirest_l2norm_bwd_f32(X, X, X, 0, 8, None) == BAD and lib.hirest_l2norm_bwd_f32(X, X, X, 2, 0, None) == BAD
    # heads_bwd(dlogits, rows, D, nheads, w0, w1, w2, dfeats): 1 <= nheads <= 3
    hb = lambda dl, rows, D, nh, w0, out: lib.hirest_heads_bwd_f32(dl, rows, D, nh, w0, X, X, out, None)
    assert hb(X, 4, 8, 0, X, X) == BAD and hb(X, 4, 8, 4, X, X) == BAD
    assert hb(None, 4, 8, 1, X, X) == BAD and hb(X, 4, 8, 1, None, X) == BAD and hb(X, 4, 8, 1, X, None) == BAD
    assert hb(X, 0, 8, 1, X, X) == BAD and hb(X, 4, 0, 1, X, X) == BAD


def test_tower_row_and_scoring_entry_points_refuse_bad_arguments_without_gpu(lib):
    """Every entry point of csrc/elementwise.hip and csrc/score.hip checks its arguments before any launch: each required pointer
    NULL in turn and each size zero or negative give HIREST_E_BADARG (-1), each documented shape rule broken once HIREST_E_SHAPE
    (-2), a two-pass top-k workspace one byte short HIREST_E_WORKSPACE (-3).  The placeholder pointers X are never dereferenced:
    each call below is refused by its checks alone.  The GPU tests of these kernels (test_gpu_tower_kernels.py) pass valid
    arguments only."""
    X = 1 << 20
    BAD, SHAPE, WS = -1, -2, -3

    def each_null(n, call, code=BAD):
        for i in range(n):
            ptrs = [X] * n
            ptrs[i] = None
            assert call(*ptrs) == code, i

    # layernorm(x, ldx, row_index, gamma, beta, eps, out, ldo, out_is_f32, rows, D): D % 4 == 0, D <= 8192, ldx % 4 == ldo % 4 == 0
    ln = lambda x, g, b, o, rows=4, D=768, ldx=768, ldo=768, f32=1: lib.hirest_layernorm(x, ldx, None, g, b, 1e-5, o, ldo, f32, rows, D, None)
    each_null(4, ln)
    assert ln(X, X, X, X, rows=0) == BAD and ln(X, X, X, X, rows=-3) == BAD
    for D in (0, -4, 6, 8196):
        assert ln(X, X, X, X, D=D, ldx=8200, ldo=8200) == SHAPE, D
        assert ln(X, X, X, X, D=D, ldx=8200, ldo=8200, f32=0, rows=9000) == SHAPE, D
    assert ln(X, X, X, X, ldx=770) == SHAPE and ln(X, X, X, X, ldo=770) == SHAPE
    # combine_hi_lo(hi, lo, ld_in, out, ldo, rows, D)
    ch = lambda hi, lo, o, rows=4, D=768, ld_in=768, ldo=768: lib.hirest_combine_hi_lo_f32(hi, lo, ld_in, o, ldo, rows, D, None)
    each_null(3, ch)
    assert ch(X, X, X, rows=0) == BAD and ch(X, X, X, rows=-1) == BAD and ch(X, X, X, D=0) == BAD and ch(X, X, X, D=-4) == BAD
    assert ch(X, X, X, D=6) == SHAPE and ch(X, X, X, ld_in=770) == SHAPE and ch(X, X, X, ldo=770) == SHAPE
    # rowstats(x, ldx, xb, stats, eps, rows, D, guard) / rowstats_split(x, ldx, xb, xlo, stats, ...): D % 4 == 0, D <= 1536; xlo, guard optional
    rs = lambda x, xb, st, rows=4, D=768, ldx=768: lib.hirest_rowstats_bf16(x, ldx, xb, st, 1e-6, rows, D, None, None)
    rs2 = lambda x, xb, st, rows=4, D=768, ldx=768: lib.hirest_rowstats_split_bf16(x, ldx, xb, X, st, 1e-6, rows, D, X, None)
    for fn in (rs, rs2):
        each_null(3, fn)
        assert fn(X, X, X, rows=0) == BAD and fn(X, X, X, rows=-1) == BAD
        for D in (0, -4, 6, 1540):
            assert fn(X, X, X, D=D, ldx=1544) == SHAPE, D
        assert fn(X, X, X, ldx=770) == SHAPE
    # ln_stats_finalize(partials, groups, stats, eps, rows, D, guard)
    fz = lambda p, st, groups=44, rows=4, D=1408: lib.hirest_ln_stats_finalize(p, groups, st, 1e-6, rows, D, None, None)
    each_null(2, fz)
    for kw in ({"groups": 0}, {"groups": -1}, {"rows": 0}, {"rows": -1}, {"D": 0}, {"D": -4}):
        assert fz(X, X, **kw) == BAD, kw
    # patchify(frames, in_dtype, B, S, P, mean3, std3, patches, Kpad): S % P == 0, Kpad % 8 == 0, Kpad >= 3 P P; dtype 2 needs mean / std
    pf = lambda fr, out, dt=0, B=2, S=224, P=14, Kpad=640, m=X, s=X: lib.hirest_patchify(fr, dt, B, S, P, m, s, out, Kpad, None)
    each_null(2, pf)
    for kw in ({"B": 0}, {"B": -1}, {"S": 0}, {"S": -224}, {"P": 0}, {"P": -14}, {"dt": 3}, {"dt": -1}, {"dt": 2, "m": None}, {"dt": 2, "s": None}):
        assert pf(X, X, **kw) == BAD, kw
    for kw in ({"S": 225}, {"Kpad": 636}, {"Kpad": 584}, {"P": 16, "Kpad": 760}):
        assert pf(X, X, **kw) == SHAPE, kw
    # fold_layernorm(W, gamma, beta, bias, Wf, bias_out, colsum_out, N, K): bias optional
    fl = lambda W, g, b, Wf, bo, so, N=8, K=768: lib.hirest_fold_layernorm(W, g, b, None, Wf, bo, so, N, K, None)
    each_null(6, fl)
    for kw in ({"N": 0}, {"N": -1}, {"K": 0}, {"K": -1}):
        assert fl(X, X, X, X, X, X, **kw) == BAD, kw
    # write_cls_rows(x, ldx, cls, pos0, B, tokens_per_frame, D)
    wc = lambda x, c, p, B=2, T=257, D=768, ldx=768: lib.hirest_write_cls_rows(x, ldx, c, p, B, T, D, None)
    each_null(3, wc)
    for kw in ({"B": 0}, {"B": -1}, {"T": 0}, {"T": -1}, {"D": 0}, {"D": -4}):
        assert wc(X, X, X, **kw) == BAD, kw
    assert wc(X, X, X, D=6) == SHAPE and wc(X, X, X, ldx=770) == SHAPE
    # embed_tokens(tokens, tok_emb, pos, x, eot_row, B, L, D, vocab): eot_row optional; vocab <= 0 would clamp ids in front of the table
    et = lambda t, e, p, x, B=2, L=77, D=512, vocab=49408: lib.hirest_embed_tokens(t, e, p, x, None, B, L, D, vocab, None)
    each_null(4, et)
    for kw in ({"B": 0}, {"B": -1}, {"L": 0}, {"L": -1}, {"D": 0}, {"D": -4}, {"vocab": 0}, {"vocab": -1}):
        assert et(X, X, X, X, **kw) == BAD, kw
    assert et(X, X, X, X, D=6) == SHAPE
    assert et(X, X, X, X, B=65536, L=32768) == SHAPE and et(X, X, X, X, B=2 ** 31 - 1, L=2 ** 31 - 1) == SHAPE    # B * L > INT32_MAX
    # f32_to_bf16(in, out, n): n % 4 == 0
    each_null(2, lambda a, b: lib.hirest_f32_to_bf16(a, b, 8, None))
    assert lib.hirest_f32_to_bf16(X, X, 0, None) == BAD and lib.hirest_f32_to_bf16(X, X, -4, None) == BAD
    assert lib.hirest_f32_to_bf16(X, X, 6, None) == SHAPE
    # pool_l2norm(frame_embeds, out, V, F, E, normalize_frames_first): E % 4 == 0, F <= 8192
    pl = lambda fe, o, V=3, F=32, E=1024: lib.hirest_pool_l2norm(fe, o, V, F, E, 0, None)
    each_null(2, pl)
    for kw in ({"V": 0}, {"V": -1}, {"F": 0}, {"F": -1}, {"E": 0}, {"E": -4}):
        assert pl(X, X, **kw) == BAD, kw
    assert pl(X, X, E=6) == SHAPE and pl(X, X, F=8193) == SHAPE
    # pool_l2norm_varlen(rows, seg_off, out, V, E)
    pv = lambda r, s, o, V=3, E=384: lib.hirest_pool_l2norm_varlen(r, s, o, V, E, None)
    each_null(3, pv)
    for kw in ({"V": 0}, {"V": -1}, {"E": 0}, {"E": -4}):
        assert pv(X, X, X, **kw) == BAD, kw
    assert pv(X, X, X, E=6) == SHAPE
    # similarity(text_n, video_n, scores, Q, V, E)
    sm = lambda t, v, s, Q=3, V=5, E=1024: lib.hirest_similarity_f32(t, v, s, Q, V, E, None)
    each_null(3, sm)
    for kw in ({"Q": 0}, {"Q": -1}, {"V": 0}, {"V": -1}, {"E": 0}, {"E": -1}):
        assert sm(X, X, X, **kw) == BAD, kw
    # topk(scores, tie_rank, Q, V, k, out_index, out_score): tie_rank, out_score optional; 1 <= k <= V
    tk = lambda s, oi, Q=3, V=100, k=10: lib.hirest_topk_f32(s, None, Q, V, k, oi, None, None)
    tw = lambda s, oi, Q=3, V=100, k=10, ws=X, nb=1 << 30: lib.hirest_topk_f32_ws(s, None, Q, V, k, oi, None, ws, nb, None)
    for fn in (tk, tw):
        each_null(2, fn)
        for kw in ({"Q": 0}, {"Q": -1}, {"V": 0}, {"V": -1}, {"k": 0}, {"k": -1}, {"k": 101}):
            assert fn(X, X, **kw) == BAD, kw
    for dims in ((0, 100, 10), (3, 0, 10), (3, 100, 0), (-1, 100, 10)):
        assert lib.hirest_topk_workspace_bytes(*dims) == BAD, dims
    assert lib.hirest_topk_workspace_bytes(5, 152620, 5) == 5 * 38 * 5 * 12          # (score, tie key, index) per chunk candidate
    need = lib.hirest_topk_workspace_bytes(3, 16387, 10)                              # five chunks: the two-pass form
    assert need == 3 * 5 * 10 * 12
    assert tw(X, X, V=16387, nb=need - 1) == WS and tw(X, X, V=16387, ws=None, nb=need) == WS and tw(X, X, V=16387, nb=0) == WS
    assert tw(X, X, V=12289, nb=3 * 4 * 10 * 12 - 1) == WS                            # four chunks: the first length that needs it
    # clip_score(img_rows, img_dtype, U, txt_rows, txt_dtype, sel, C, K, E, out)
    cs = lambda img, txt, sel, out, idt=0, tdt=1, U=8, C=4, K=3, E=512: lib.hirest_clip_score(img, idt, U, txt, tdt, sel, C, K, E, out, None)
    each_null(4, cs)
    for kw in ({"idt": 2}, {"idt": -1}, {"tdt": 2}, {"U": 0}, {"C": -1}, {"K": 0}, {"E": 0}):
        assert cs(X, X, X, X, **kw) == BAD, kw


def test_workspace_size_formula(lib):
    from hirest_amd import _lib
    t = _lib.VisionTower()
    t.image_size, t.patch, t.width, t.heads, t.head_dim, t.mlp_dim, t.layers, t.embed_dim, t.kpad = 224, 14, 1408, 16, 88, 6144, 40, 1024, 640
    M = 256 * 257
    al = lambda v: (v + 255) // 256 * 256
    assert lib.hirest_vision_workspace_bytes(ctypes.byref(t), 256) == al(M * 1408 * 4) + al(M * 1408 * 2) + al(M * 6144 * 2) + al(256 * 4)


def test_model_schema_and_errors():
    import hirest_amd
    from hirest_amd import synth
    with pytest.raises(RuntimeError):
        hirest_amd.build_eva_model_and_transforms("no-such-model", pretrained="synth:0")
    with pytest.raises(Exception):
        hirest_amd.build_eva_model_and_transforms("EVA_CLIP_tiny_test", pretrained="/nonexistent.pt")
    model, pre = hirest_amd.build_eva_model_and_transforms("EVA_CLIP_tiny_test", pretrained="synth:11", precision="bf16")
    assert model.training  # the reference returns a train-mode module (eva_clip.py:155-172)
    sd = synth.eva_clip_state_dict(synth.EVA_CLIP_TINY, 11)
    got = model.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert model.visual.image_size == 224 and model.visual.image_mean == hirest_amd.eva_clip.OPENAI_DATASET_MEAN
    for p in model.parameters():
        p.requires_grad = False           # modeling.py:126-129 freeze loop works
    assert sum(p.numel() for p in model.parameters()) == sum(v.numel() for v in sd.values())
    with pytest.raises(AssertionError):   # vit_model.py:203
        model.encode_image(torch.zeros(1, 3, 200, 224))
    with pytest.raises(RuntimeError):     # no silent CPU fallback
        model.encode_image(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError):
        model.encode_text(torch.zeros(1, 77, dtype=torch.long))
    # checkpoint round trip incl. the 'module.' prefix + wrapper keys (eva_clip.py:68-79)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ck.pt")
        torch.save({"model": {"module." + k: v for k, v in sd.items()}}, path)
        m2, _ = hirest_amd.build_eva_model_and_transforms("EVA_CLIP_tiny_test", pretrained=path)
        assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)


def test_eva_g14_param_count():
    """1 012 588 928 vision + 123 846 913 text params, without allocating them."""
    from hirest_amd import synth
    nv = sum(int(np.prod(s)) for s in synth.eva_vision_shapes(synth.EVA_CLIP_G_14).values())
    nt = sum(int(np.prod(s)) if len(s) else 1 for s in synth.eva_text_shapes(synth.EVA_CLIP_G_14).values())
    assert nv == 1012588928 and nt == 123846913


def test_image_transform_geometry():
    from PIL import Image
    import hirest_amd
    tf = hirest_amd.image_transform(224)
    rng = np.random.RandomState(0)
    for (h, w) in [(300, 400), (400, 300), (224, 224), (225, 1000)]:
        img = Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8))
        t = tf(img)
        assert t.shape == (3, 224, 224) and t.dtype == torch.float32
    # a 224x224 image is only converted + normalised: exact formula check
    arr = rng.randint(0, 255, (224, 224, 3), dtype=np.uint8)
    t = tf(Image.fromarray(arr))
    mean = np.array(hirest_amd.eva_clip.OPENAI_DATASET_MEAN, dtype=np.float32).reshape(3, 1, 1)
    std = np.array(hirest_amd.eva_clip.OPENAI_DATASET_STD, dtype=np.float32).reshape(3, 1, 1)
    want = (arr.astype(np.float32).transpose(2, 0, 1) / 255.0 - mean) / std
    assert np.allclose(t.numpy(), want, atol=1e-6)


def test_moment_model_builds_its_own_clip_like_the_reference(tmp_path, monkeypatch):
    """modeling.py:115-129: MomentModel(n_frames, asr_dim, args) builds EVA_CLIP_g_14 from ./pretrained_weights/
    eva_clip_psz14.pt, casts to float, puts it in eval mode and freezes it.  Offline the two args fields redirect the build
    to a synthetic checkpoint of the tiny towers; without them the reference's file is looked for and its absence is the
    reference's error."""
    import hirest_amd
    from hirest_amd import synth

    class Args:
        clip_model_name = "EVA_CLIP_tiny_e1024_test"
        clip_pretrained = "synth:11"
    m = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=Args())
    assert isinstance(m.clip_model, hirest_amd.EVA_CLIP) and not m.clip_model.training
    assert all(not p.requires_grad for p in m.clip_model.parameters())
    assert all(p.dtype == torch.float32 for p in m.clip_model.parameters())
    assert any(p.requires_grad for n, p in m.named_parameters() if not n.startswith("clip_model."))
    sd = m.state_dict()
    assert "clip_model.text.token_embedding.weight" in sd and "clip_model.visual.blocks.0.attn.q_bias" in sd
    want = synth.eva_clip_state_dict(dict(synth.EVA_CLIP_TINY, embed_dim=1024), 11)
    assert torch.equal(sd["clip_model.text.text_projection"], want["text.text_projection"])
    assert m.clip_preprocess is not None
    with pytest.raises(RuntimeError):                       # no CPU fallback: the text tower refuses host tensors
        m.test_step({"tasks": ["moment_retrieval"], "clip_text_ids": torch.zeros(1, 77, dtype=torch.long),
                     "vis_feats": torch.zeros(1, 4, 1024), "vis_mask": torch.ones(1, 4, dtype=torch.long),
                     "moment_mask": torch.ones(1, 4, dtype=torch.long), "asr_feats": torch.zeros(1, 4, 384)})
    monkeypatch.chdir(tmp_path)                             # no ./pretrained_weights here
    with pytest.raises(FileNotFoundError):
        hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=None)
    assert hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=None, clip_model=None).clip_model is None


def test_profiled_kernels_are_the_dispatched_ones(lib):
    """a committed profile must describe kernels the library launches TODAY.  Every gemm_* instantiation named in
    the newest profiles/rNN/pmc_traffic.json and pmc_summary.md (section 1: the bench's kernels) has to be what
    hirest_gemm_dispatch_name returns for one of the tower's problems under the default selection; and bench.py's roofline
    looks its traffic figure up in that same directory."""
    import json
    from hirest_amd import _lib

    def name(M, N, K, epi):
        a = _lib.GemmArgs.make(1, K, 1, K, None, 1, N, M, N, K, epi)
        buf = ctypes.create_string_buffer(64)
        assert lib.hirest_gemm_dispatch_name(ctypes.byref(a), buf, 64) == 0
        return buf.value.decode()
    lib.hirest_gemm_select_kernel(0)
    lib.hirest_gemm_debug_mode(0)
    Mv, Mp, Mt = 1024 * 257, 1024 * 256, 546 * 77
    problems = [(Mv, 4224, 1408, _lib.EPI_LNFOLD_BF16), (Mv, 1408, 1408, _lib.EPI_BIAS_RESID2_LNSTATS),
                (Mv, 6144, 1408, _lib.EPI_LNFOLD_GELU_BF16), (Mv, 1408, 6144, _lib.EPI_BIAS_RESID2_LNSTATS),
                # (HIREST_TOWER_F32_RESIDUAL: the fp32 residual array of rounds 1-3)
                (Mv, 1408, 1408, _lib.EPI_BIAS_RESID_LNSTATS_F32), (Mv, 1408, 6144, _lib.EPI_BIAS_RESID_LNSTATS_F32),
                (Mp, 1408, 640, _lib.EPI_PATCH_POS_F32), (1024, 1024, 1408, _lib.EPI_BIAS_F32),
                # text tower (546 prompts x 77 tokens, width 768): qkv, out_proj, c_fc, c_proj, projection
                (Mt, 2304, 768, _lib.EPI_BIAS_BF16), (Mt, 768, 768, _lib.EPI_BIAS_RESID_F32), (Mt, 3072, 768, _lib.EPI_BIAS_GELU_BF16),
                (Mt, 768, 3072, _lib.EPI_BIAS_RESID_F32), (546, 1024, 768, _lib.EPI_BIAS_F32)]
    dispatched = {name(*p) for p in problems}
    assert {"gemm_pq256<7>", "gemm_pq256<10>", "gemm_pq256<6>", "gemm_pq256<8>", "gemm_pq256<5>"} <= dispatched        # (round 4: the two-phase ping-pong kernel)
    rounds = sorted(d for d in os.listdir(os.path.join(REPO, "profiles")) if re.fullmatch(r"r\d\d", d))
    # the newest round that holds a traffic profile (a round's directory exists from its first committed measurement on; its
    # counters are collected on the final build)
    with_traffic = [r for r in rounds if os.path.isfile(os.path.join(REPO, "profiles", r, "pmc_traffic.json"))]
    if with_traffic[-1] != rounds[-1]:
        pytest.skip(f"profiles/{rounds[-1]} has no traffic profile yet (collected on the round's final build: tools/final_round.sh)")
    newest = os.path.join(REPO, "profiles", with_traffic[-1])
    src = open(os.path.join(REPO, "bench.py")).read()
    assert f'"{rounds[-1]}"' in src.split("PROFILE_ROUNDS")[1].split("\n")[0]      # bench.py reads the newest round first
    prof = json.load(open(os.path.join(newest, "pmc_traffic.json")))
    named = set()
    for k in prof["kernels"]:
        named |= set(re.findall(r"gemm_\w+<[^>]*>", k["kernel"]))
    sec1 = open(os.path.join(newest, "pmc_summary.md")).read().split("## 2.")[0]
    named |= set(re.findall(r"`(gemm_\w+<[^>`]*>)`", sec1))
    assert named, "no GEMM kernels found in the newest profile"
    assert named <= dispatched, f"profiled but no longer dispatched: {sorted(named - dispatched)}"
    # selection switches change the answer (the entry point mirrors the dispatch, it is not a constant table)
    lib.hirest_gemm_select_kernel(6)
    assert name(Mv, 1408, 6144, _lib.EPI_BIAS_RESID_LNSTATS_F32) == "gemm_p256<6, 64, false, 1>"
    for retired in (10, 17, 18, 20):                                      # the 4-wave kernel (round 2) and gemm_d2 (round 3)
        assert lib.hirest_gemm_select_kernel(retired) != 0
    lib.hirest_gemm_select_kernel(0)


# (selection, debug word, flags, M, N, K, epilogue) -> (status, name) of hirest_gemm_dispatch_name, recorded from the library of the commit
# before the launch code and the name function were given one decision function (csrc/gemm.hip: gemm_choose / gemm_kernel).  Every kernel
# family, every kind of rejection and both sides of every threshold of the decision; flags: 1 REVERSE, 2 X3, 4 X3_T128.
GEMM_DISPATCH_PIN = [
    # plain epilogues, automatic selection: t128 below M * N = 2048 * 1024, M = 512 or N = 256, pq256 from there on
    (0, 0, 0, 511, 8192, 64, 0, 0, 'gemm_t128<0>'), (0, 0, 0, 512, 4096, 64, 0, 0, 'gemm_pq256<0>'), (0, 0, 0, 512, 4092, 64, 0, 0, 'gemm_t128<0>'),
    (0, 0, 0, 8192, 252, 64, 2, 0, 'gemm_t128<2>'), (0, 0, 0, 8192, 256, 64, 2, 0, 'gemm_pq256<2>'), (0, 0, 1, 39424, 2304, 768, 0, 0, 'gemm_pq256<0>'),
    (0, 0, 4, 512, 4096, 64, 0, 0, 'gemm_pq256<0>'),                 # (X3_T128 without X3: the launch rejects it, the name does not look)
    (0, 0, 0, 262144, 1408, 640, 5, 0, 'gemm_pq256<5>'),
    # debug word: bit 9 alone changes nothing, bits 10-19 take the measurement variant, the others p256's DBG instantiation where it exists
    (0, 512, 0, 512, 4096, 64, 1, 0, 'gemm_pq256<1>'), (0, 1024, 0, 512, 4096, 64, 0, 0, 'gemm_pq256_dbg<0>'),
    (0, 262144, 0, 263168, 1408, 6144, 10, 0, 'gemm_pq256_dbg<10>'), (9, 4096, 0, 128, 128, 64, 4, 0, 'gemm_pq256_dbg<4>'),
    (0, 4, 0, 512, 4096, 64, 3, 0, 'gemm_p256<3, 64, true, 1>'), (0, 4, 0, 512, 4096, 64, 4, 0, 'gemm_pq256<4>'), (0, 4, 0, 511, 8192, 64, 3, 0, 'gemm_t128<3>'),
    (0, 1025, 0, 512, 4096, 64, 0, 0, 'gemm_p256<0, 64, true, 1>'),
    # forced selections
    (1, 0, 0, 4096, 4096, 64, 4, 0, 'gemm_t128<4>'), (2, 0, 0, 4096, 4096, 64, 3, 0, 'gemm_t256<3, 4>'), (3, 0, 0, 128, 128, 64, 5, 0, 'gemm_t256<5, 5>'),
    (4, 0, 0, 4096, 4096, 64, 0, 0, 'gemm_t256p<0>'), (5, 0, 0, 4096, 4096, 64, 1, 0, 'gemm_t256q<1>'), (6, 0, 0, 4096, 4096, 64, 1, 0, 'gemm_p256<1, 64, false, 1>'),
    (6, 1, 0, 4096, 4096, 64, 1, 0, 'gemm_p256<1, 64, true, 1>'), (6, 1, 0, 4096, 4096, 64, 2, 0, 'gemm_p256<2, 64, false, 1>'),
    (7, 1, 0, 4096, 4096, 64, 0, 0, 'gemm_p256<0, 128, false, 1>'), (8, 0, 0, 128, 128, 64, 2, 0, 'gemm_pp256<2, 1>'), (9, 0, 0, 128, 128, 64, 3, 0, 'gemm_pq256<3>'),
    # LN-fold epilogues: persistent kernels only, from M = 64, N = 256 on; selections other than 6 / 8 and the p256 debug bits do not apply
    (0, 0, 0, 64, 256, 64, 7, 0, 'gemm_pq256<7>'), (0, 0, 0, 63, 256, 64, 7, -2, ''), (0, 0, 0, 64, 252, 64, 8, -2, ''),
    (1, 0, 0, 263168, 1408, 1408, 10, 0, 'gemm_pq256<10>'), (0, 1, 0, 263168, 1408, 6144, 6, 0, 'gemm_pq256<6>'),
    (6, 1, 0, 263168, 1408, 6144, 6, 0, 'gemm_p256<6, 64, false, 1>'), (8, 0, 0, 263168, 4224, 1408, 7, 0, 'gemm_pp256<7, 1>'),
    (0, 65536, 0, 263168, 6144, 1408, 8, 0, 'gemm_pq256_dbg<8>'),
    # split operands: t128x3 below 256 tiles of 256 x 256 (not for GELU_SPLIT2) or under X3_T128, which also allows 192-row tiles (4 * c3 <= 3 * c2)
    (0, 0, 2, 65280, 256, 128, 4, 0, 'gemm_t128x3<4, 2>'), (0, 0, 2, 65536, 256, 128, 4, 0, 'gemm_pp256x3<4>'), (9, 0, 2, 65536, 256, 128, 3, 0, 'gemm_pq256x3<3>'),
    (0, 0, 2, 1500, 768, 1536, 9, 0, 'gemm_pp256x3<9>'), (9, 1, 2, 1500, 768, 1536, 9, 0, 'gemm_pq256x3<9>'), (0, 0, 6, 1500, 3072, 1536, 9, 0, 'gemm_t128x3<9, 3>'),
    (0, 0, 6, 1500, 768, 1536, 3, 0, 'gemm_t128x3<3, 2>'), (0, 0, 6, 192, 32768, 64, 4, 0, 'gemm_t128x3<4, 3>'), (0, 0, 6, 193, 32768, 64, 4, 0, 'gemm_t128x3<4, 2>'),
    (0, 0, 2, 192, 32768, 64, 4, 0, 'gemm_t128x3<4, 2>'), (0, 0, 6, 65536, 256, 128, 3, 0, 'gemm_t128x3<3, 2>'),
    # rejected: unknown epilogue, GELU_SPLIT2 without X3, X3 with an epilogue it has no kernel for
    (0, 0, 0, 512, 4096, 64, 11, -1, ''), (0, 0, 0, 512, 4096, 64, -1, -1, ''), (0, 0, 0, 512, 4096, 64, 9, -1, ''), (0, 0, 2, 512, 4096, 64, 0, -1, ''),
    (0, 0, 6, 512, 4096, 64, 7, -1, ''), (9, 0, 2, 512, 4096, 64, 10, -1, ''),
]


def test_gemm_dispatch_names_are_pinned(lib):
    """hirest_gemm_dispatch_name over GEMM_DISPATCH_PIN: status and string equal the recorded ones (a rejected call leaves the buffer alone)."""
    from hirest_amd import _lib
    try:
        for sel, dbg, flags, M, N, K, epi, status, name in GEMM_DISPATCH_PIN:
            assert lib.hirest_gemm_select_kernel(sel) == 0 and lib.hirest_gemm_debug_mode(dbg) == 0
            a = _lib.GemmArgs.make(1, K, 1, K, None, 1, N, M, N, K, epi)
            a.flags = flags
            buf = ctypes.create_string_buffer(64)
            got = lib.hirest_gemm_dispatch_name(ctypes.byref(a), buf, 64)
            assert (got, buf.value.decode()) == (status, name), (sel, dbg, flags, M, N, K, epi)
        # the entry point's own arguments: NULL, a buffer under 48 bytes, another struct layout
        a = _lib.GemmArgs.make(1, 64, 1, 64, None, 1, 4096, 512, 4096, 64, 0)
        assert lib.hirest_gemm_dispatch_name(ctypes.byref(a), buf, 48) == 0
        assert lib.hirest_gemm_dispatch_name(None, buf, 64) == -1 and lib.hirest_gemm_dispatch_name(ctypes.byref(a), None, 64) == -1
        assert lib.hirest_gemm_dispatch_name(ctypes.byref(a), buf, 47) == -1
        a.struct_size -= 8
        assert lib.hirest_gemm_dispatch_name(ctypes.byref(a), buf, 64) == -1
    finally:
        lib.hirest_gemm_select_kernel(0)
        lib.hirest_gemm_debug_mode(0)


def test_joint_inference_entry_points_refuse_bad_arguments_without_gpu(lib):
    """The inference entry points of the joint model (csrc/joint.hip, csrc/caption.hip) check their arguments before any launch:
    NULL pointers, non-positive sizes, E or D not a positive multiple of 4, nheads outside 1..3 or a missing weight of a used head,
    T > 16384 for segmentation_step, a beam wider than 16 for the tail and a decode step without any key give HIREST_E_BADARG (-1);
    an attention head width that is not a multiple of 4 up to 96 and row strides that are not multiples of 4 HIREST_E_SHAPE (-2).
    The placeholder pointers X are never dereferenced: each call below is refused by its checks alone."""
    X = 1 << 20
    BAD, SHAPE, WS = -1, -2, -3
    # joint_time_grid(n_valid, B, T, grid)
    assert lib.hirest_joint_time_grid_f32(X, 5, 300, None, None) == BAD
    assert lib.hirest_joint_time_grid_f32(X, 0, 300, X, None) == BAD and lib.hirest_joint_time_grid_f32(X, 5, 0, X, None) == BAD
    # joint_time_features(n_valid, w1, b1, tin, B, T, E)
    for i in range(4):
        ptrs = [X] * 4
        ptrs[i] = None
        assert lib.hirest_joint_time_features(*ptrs, 2, 300, 512, None) == BAD, i
    for dims in ((0, 300, 512), (2, 0, 512), (2, 300, 0), (2, 300, 514), (2, 300, -4)):
        assert lib.hirest_joint_time_features(X, X, X, X, *dims, None) == BAD, dims
    # joint_base(v, text_proj, asr, temporal, base, B, T, E)
    for i in range(5):
        ptrs = [X] * 5
        ptrs[i] = None
        assert lib.hirest_joint_base(*ptrs, 2, 300, 512, None) == BAD, i
    for dims in ((0, 300, 512), (2, 0, 512), (2, 300, 0), (2, 300, 6), (2, 300, -8)):
        assert lib.hirest_joint_base(X, X, X, X, X, *dims, None) == BAD, dims
    # joint_mask_add(base, moment_mask, boundary_mask, mask_embed, boundary_embed, f, rows, E): a boundary mask needs its table
    for i in (0, 1, 3, 5):
        ptrs = [X] * 6
        ptrs[i] = None
        assert lib.hirest_joint_mask_add(*ptrs, 600, 512, None) == BAD, i
    assert lib.hirest_joint_mask_add(X, X, X, X, None, X, 600, 512, None) == BAD
    for rows, E in ((0, 512), (600, 0), (600, 510), (600, -4)):
        assert lib.hirest_joint_mask_add(X, X, None, X, None, X, rows, E, None) == BAD, (rows, E)
    # linear_heads(x, rows, D, nheads, w0, w1, w2, bias3, logits)
    lh = lambda x, rows, D, nh, w0, w1, w2, b, out: lib.hirest_linear_heads(x, rows, D, nh, w0, w1, w2, b, out, None)
    assert lh(None, 4, 8, 1, X, None, None, X, X) == BAD and lh(X, 4, 8, 1, None, None, None, X, X) == BAD
    assert lh(X, 4, 8, 1, X, None, None, None, X) == BAD and lh(X, 4, 8, 1, X, None, None, X, None) == BAD
    assert lh(X, 4, 8, 0, X, X, X, X, X) == BAD and lh(X, 4, 8, 4, X, X, X, X, X) == BAD
    assert lh(X, 4, 8, 2, X, None, X, X, X) == BAD and lh(X, 4, 8, 3, X, X, None, X, X) == BAD
    assert lh(X, 0, 8, 1, X, None, None, X, X) == BAD and lh(X, 4, 0, 1, X, None, None, X, X) == BAD
    assert lh(X, 4, 6, 1, X, None, None, X, X) == BAD and lh(X, 4, -4, 1, X, None, None, X, X) == BAD
    # masked_argmax(logits, mask, fill, B, T, out)
    assert lib.hirest_masked_argmax(None, X, -1e10, 2, 300, X, None) == BAD and lib.hirest_masked_argmax(X, None, -1e10, 2, 300, X, None) == BAD
    assert lib.hirest_masked_argmax(X, X, -1e10, 2, 300, None, None) == BAD
    assert lib.hirest_masked_argmax(X, X, -1e10, 0, 300, X, None) == BAD and lib.hirest_masked_argmax(X, X, -1e10, 2, 0, X, None) == BAD
    # segmentation_step(logits, moment_mask, boundary_mask, B, T, threshold, steps, nsteps, max_steps, probs_out)
    seg = lambda lg, mm, bm, B, T, st, ns: lib.hirest_segmentation_step(lg, mm, bm, B, T, 0.5, st, ns, 20, None, None)
    for i in range(5):
        ptrs = [X] * 5
        ptrs[i] = None
        assert seg(ptrs[0], ptrs[1], ptrs[2], 2, 300, ptrs[3], ptrs[4]) == BAD, i
    assert seg(X, X, X, 0, 300, X, X) == BAD and seg(X, X, X, 2, 0, X, X) == BAD
    assert seg(X, X, X, 2, 16385, X, X) == BAD
    # attention_f32(qkv, out, B, T, H, dh) / attention_f32_varlen(qkv, out, seq_off, B, max_len, H, dh)
    af = lambda q, o, B, T, H, dh: lib.hirest_attention_f32(q, o, B, T, H, dh, 0.125, 0.0, None)
    assert af(None, X, 1, 64, 2, 64) == BAD and af(X, None, 1, 64, 2, 64) == BAD
    assert af(X, X, 0, 64, 2, 64) == BAD and af(X, X, 1, 0, 2, 64) == BAD and af(X, X, 1, 64, 0, 64) == BAD
    for dh in (0, -4, 6, 100):
        assert af(X, X, 1, 64, 2, dh) == SHAPE, dh
    av = lambda q, o, so, B, L, dh: lib.hirest_attention_f32_varlen(q, o, so, B, L, 12, dh, 0.125, 0.0, None)
    assert av(X, X, None, 3, 40, 32) == BAD and av(X, None, X, 3, 40, 32) == BAD
    assert av(X, X, X, 0, 40, 32) == BAD and av(X, X, X, 3, 0, 32) == BAD
    assert av(X, X, X, 3, 40, 30) == SHAPE and av(X, X, X, 3, 40, 128) == SHAPE
    # attention_f32_qkv(q, ldq, k, v, ldkv, out, B, Tq, Tk, H, dh, scale, add_const, causal_penalty)
    aq = lambda q, ldq, k, v, ldkv, o, B, Tq, Tk, H, dh: lib.hirest_attention_f32_qkv(q, ldq, k, v, ldkv, o, B, Tq, Tk, H, dh, 0.125, 0.0,
                                                                                      -1e30, None)
    for i in range(4):
        ptrs = [X] * 4
        ptrs[i] = None
        assert aq(ptrs[0], 128, ptrs[1], ptrs[2], 256, ptrs[3], 1, 17, 300, 2, 64) == BAD, i
    for dims in ((0, 17, 300, 2), (1, 0, 300, 2), (1, 17, 0, 2), (1, 17, 300, 0)):
        assert aq(X, 128, X, X, 256, X, *dims, 64) == BAD, dims
    assert aq(X, 130, X, X, 256, X, 1, 17, 300, 2, 64) == SHAPE and aq(X, 128, X, X, 258, X, 1, 17, 300, 2, 64) == SHAPE
    assert aq(X, 128, X, X, 256, X, 1, 17, 300, 2, 66) == SHAPE and aq(X, 256, X, X, 512, X, 1, 17, 300, 2, 100) == SHAPE
    # attention_f32_decode(q, ldq, k_hist, v_hist, ld_hist, parent, t_hist, k_new, v_new, ld_new, k_out, v_out, out, R, H)
    ad = lambda q, ldq, kh, vh, ldh, th, kn, vn, ldn, ko, vo, o, R, H: lib.hirest_attention_f32_decode(
        q, ldq, kh, vh, ldh, None, th, kn, vn, ldn, ko, vo, o, R, H, 0.125, 0.0, 0.0, None)
    assert ad(X, 384, None, None, 128, 0, None, None, 384, None, None, X, 6, 2) == BAD          # no history and no new key
    assert ad(None, 384, X, X, 128, 5, X, X, 384, X, X, X, 6, 2) == BAD and ad(X, 384, X, X, 128, 5, X, X, 384, X, X, None, 6, 2) == BAD
    assert ad(X, 384, X, X, 128, 5, X, X, 384, X, X, X, 0, 2) == BAD and ad(X, 384, X, X, 128, 5, X, X, 384, X, X, X, 6, 0) == BAD
    assert ad(X, 384, X, X, 128, -1, X, X, 384, X, X, X, 6, 2) == BAD
    assert ad(X, 384, None, X, 128, 5, X, X, 384, X, X, X, 6, 2) == BAD and ad(X, 384, X, None, 128, 5, X, X, 384, X, X, X, 6, 2) == BAD
    assert ad(X, 384, X, X, 128, 5, X, None, 384, X, X, X, 6, 2) == BAD and ad(X, 384, X, X, 128, 5, X, X, 384, X, None, X, 6, 2) == BAD
    assert ad(X, 386, X, X, 128, 5, X, X, 384, X, X, X, 6, 2) == SHAPE and ad(X, 384, X, X, 130, 5, X, X, 384, X, X, X, 6, 2) == SHAPE
    assert ad(X, 384, X, X, 128, 5, X, X, 386, X, X, X, 6, 2) == SHAPE
    # caption_beam_tail(logits, ldx, row_add, B, beam, vocab, step, max_steps, eos, scores, tokens, backptr, n_steps, done, next_ids,
    #                   next_parents, next_add, done_host, workspace, workspace_bytes)
    big = 1 << 30
    bt = lambda ldx, B, beam, V, step, wsb=big, logits=X: lib.hirest_caption_beam_tail(logits, ldx, X, B, beam, V, step, 48, 102, X, X, X, X, X, X,
                                                                                        X, X, None, X, wsb, None)
    assert bt(30528, 5, 17, 30528, 0) == BAD and bt(30528, 5, 0, 30528, 0) == BAD and bt(30528, 0, 5, 30528, 0) == BAD
    assert bt(30528, 5, 5, 30528, 48) == BAD and bt(30528, 5, 5, 30528, -1) == BAD and bt(30528, 5, 5, 0, 0) == BAD
    assert bt(30528, 5, 5, 30528, 0, logits=None) == BAD
    assert bt(30522, 5, 5, 30522, 0) == SHAPE and bt(30530, 5, 5, 30528, 0) == SHAPE and bt(30528, 5, 5, 30528, 0, logits=X + 4) == SHAPE
    assert bt(8, 5, 12, 8, 0) == SHAPE and bt(32772, 5, 5, 32772, 0) == SHAPE                   # beam > vocab, vocab > 32768
    assert bt(30528, 5, 5, 30528, 0, wsb=lib.hirest_caption_beam_tail_workspace_bytes(5, 5, 30528) - 1) == WS
    # beam_advance(val, idx, B, beam, vocab, step, max_steps, eos, ...) / beam_backtrack(scores, tokens, backptr, n_steps, B, beam, max_steps, out)
    ba = lambda B, beam, step: lib.hirest_beam_advance(X, X, B, beam, 30528, step, 48, 102, X, X, X, X, X, X, X, X, None)
    assert ba(5, 65, 0) == BAD and ba(5, 0, 0) == BAD and ba(0, 5, 0) == BAD and ba(5, 5, 48) == BAD and ba(5, 5, -1) == BAD
    bb = lambda s, t, bp, n, B, beam, ms, o: lib.hirest_beam_backtrack(s, t, bp, n, B, beam, ms, o, None)
    for i in range(5):
        ptrs = [X] * 5
        ptrs[i] = None
        assert bb(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 5, 5, 48, ptrs[4]) == BAD, i
    assert bb(X, X, X, X, 0, 5, 48, X) == BAD and bb(X, X, X, X, 5, 0, 48, X) == BAD and bb(X, X, X, X, 5, 5, 0, X) == BAD
    # log_softmax(x, ldx, row_add, out, ldo, rows, V)
    assert lib.hirest_log_softmax_f32(None, 8, None, X, 8, 2, 8, None) == BAD and lib.hirest_log_softmax_f32(X, 8, None, None, 8, 2, 8, None) == BAD
    assert lib.hirest_log_softmax_f32(X, 8, None, X, 8, 0, 8, None) == BAD and lib.hirest_log_softmax_f32(X, 8, None, X, 8, 2, 0, None) == BAD


def test_stream_workspace_is_keyed_by_stream_and_retires_outgrown_buffers():
    """ops.stream_workspace on the CPU with explicit stream keys: one buffer per (device, tag, stream); a request that fits returns the
    same buffer; a larger one gets a new buffer of at least twice the size while the old tensor stays referenced (work still in flight on
    that stream may be reading it) and no other key's buffer moves."""
    from hirest_amd import ops
    cpu, MB = torch.device("cpu"), 1 << 20
    s1, s2 = 0x7001, 0x7002                                 # stand-ins for raw stream pointers
    tag = "test_stream_workspace"                           # this test's own buffers
    assert ops.stream_workspace(cpu, 0, tag, s1) == (None, 0) and ops.stream_workspace(cpu, -5, tag, s1) == (None, 0)
    p1, n1 = ops.stream_workspace(cpu, 1000, tag, s1)
    p2, n2 = ops.stream_workspace(cpu, 1000, tag, s2)
    assert p1 != p2 and n1 == n2 == 32 * MB                 # the minimum size
    assert ops.stream_workspace(cpu, n1, tag, s1) == (p1, n1) and ops.stream_workspace(cpu, 1, tag, s1) == (p1, n1)
    po, no = ops.stream_workspace(cpu, 1000, tag + ".other", s1)        # another tag on the same stream
    assert po not in (p1, p2) and no == 32 * MB
    old = ops._STREAM_WS[("cpu", None, tag, s1)]
    retired = len(ops._STREAM_WS_RETIRED)
    q1, m1 = ops.stream_workspace(cpu, n1 + 1, tag, s1)
    assert q1 != p1 and m1 >= 2 * n1
    assert len(ops._STREAM_WS_RETIRED) == retired + 1 and ops._STREAM_WS_RETIRED[-1] is old and old.data_ptr() == p1 and old.numel() == n1
    assert ops.stream_workspace(cpu, 1000, tag, s2) == (p2, n2)          # the other stream's buffer is untouched
    assert ops.stream_workspace(cpu, 1000, tag + ".other", s1) == (po, no)
    assert ops.stream_workspace(cpu, 1000, tag, s1) == (q1, m1)
