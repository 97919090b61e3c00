"""Tensor-level wrappers over the C ABI (one function per kernel entry point).

torch is used for device memory and the current stream only; every computation below is a
hand-written gfx950 kernel inside libhirest_hip.so.  All wrappers validate device / dtype /
contiguity and raise RuntimeError on violations (the reference's ATen ops raise likewise).
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_BIAS_BF16, EPI_BIAS_F32, EPI_BIAS_GELU_BF16, EPI_BIAS_QGELU_BF16, EPI_BIAS_RESID_F32,
                   EPI_PATCH_POS_F32)

__all__ = ["gemm", "layernorm", "attention", "patchify", "write_cls_rows", "embed_tokens", "to_bf16",
           "pool_l2norm", "similarity", "topk", "clip_score", "stream_ptr", "on_tensor_device"]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr() -> int:
    """Raw hipStream_t of torch's current stream on the CURRENT device (wrappers switch to their tensors' device first).  Called
    once per kernel launch — the training step issues ~300 per iteration from Python — so it takes torch's raw accessor when the
    build has it (no Stream object per call)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def on_tensor_device(fn):
    """Run `fn` with the device of its first GPU tensor argument current.  The reference's drivers place models with
    ``.to(device)`` and never call ``set_device`` (run.py:61-65, inference_video_retrieval.py:195-201); a kernel must
    then launch on the stream — and with the per-device kernel attributes — of the tensors' device, not of cuda:0."""
    @functools.wraps(fn)
    def wrapped(*args, **kw):
        for a in list(args) + list(kw.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kw)
                break
        return fn(*args, **kw)
    return wrapped


def _dev(t: torch.Tensor, dtype, name: str) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], dtype, name: str) -> Optional[int]:
    return None if t is None else _dev(t, dtype, name)


@on_tensor_device
def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, epilogue: int,
         pos: Optional[torch.Tensor] = None, patches_per_frame: int = 0,
         aux0: Optional[torch.Tensor] = None, aux1: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
    """out <- epilogue(a @ w.T + bias); a [M,K] bf16, w [N,K] bf16, bias [N] f32.  aux0 / aux1: the LN-fold epilogues'
    extra operands (include/hirest_hip.h)."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise RuntimeError(f"gemm: K mismatch {a.shape} x {w.shape}")
    out_dtype = torch.bfloat16 if epilogue in (EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_QGELU_BF16, _lib.EPI_LNFOLD_BF16,
                                              _lib.EPI_LNFOLD_GELU_BF16, _lib.EPI_BIAS_RESID2_LNSTATS) else torch.float32
    args = _lib.GemmArgs.make(_dev(a, torch.bfloat16, "gemm.a"), K, _dev(w, torch.bfloat16, "gemm.w"), K,
                         _opt(bias, torch.float32, "gemm.bias"), _dev(out, out_dtype, "gemm.out"), out.shape[-1],
                         M, N, K, epilogue, _opt(pos, torch.float32, "gemm.pos"), patches_per_frame,
                         None if aux0 is None else _dev(aux0, aux0.dtype, "gemm.aux0"),
                         None if aux1 is None else _dev(aux1, aux1.dtype, "gemm.aux1"), int(flags))
    _lib.check(lib.hirest_gemm_bf16(C.byref(args), stream_ptr()), "hirest_gemm_bf16")
    return out


def gemm_select_kernel(which: int):
    """Which bf16 GEMM kernel hirest_gemm_bf16 launches (include/hirest_hip.h: hirest_gemm_select_kernel; tests and A/B timing):
    0 = automatic (pq256 for M * N >= 2^21 with M >= 512 and N >= 256 and for every LN-fold epilogue, the 128x128 kernel below that),
    1 = the 128x128 kernel (t128), 2 / 3 = the 256x256 ping-pong kernel with a 4- / 5-slot LDS ring (t256), 4 = t256p (32-deep slabs),
    5 = t256q (64-deep steps), 6 / 7 = the persistent 256x256 kernel with 8 / 4 waves (p256), 8 = the persistent ping-pong kernel (pp256),
    9 = pp256 with two phases per 64-deep step (pq256, and pq256x3 for HIREST_GEMM_X3).  Same bits for every selection."""
    _lib.check(_lib.load().hirest_gemm_select_kernel(int(which)), "hirest_gemm_select_kernel")


ATTENTION_DEFAULT_KERNEL = 7     # persistent kernel + producer wave (include/hirest_hip.h: hirest_attention_select_kernel)


def attention_select_kernel(which: int):
    _lib.check(_lib.load().hirest_attention_select_kernel(int(which)), "hirest_attention_select_kernel")


def attention_set_mapping(by_head: Optional[bool] = None):
    """Persistent attention kernel: one head per workgroup over frames (True), one frame per workgroup (False), or automatic (None, the
    default: by head below 256 frames)."""
    _lib.check(_lib.load().hirest_attention_set_mapping(2 if by_head is None else int(bool(by_head))), "hirest_attention_set_mapping")


@on_tensor_device
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor,
              row_index: Optional[torch.Tensor] = None, ldx: Optional[int] = None, rows: Optional[int] = None):
    lib = _lib.load()
    D = gamma.numel()
    rows = rows if rows is not None else (row_index.numel() if row_index is not None else x.numel() // D)
    ldx = ldx if ldx is not None else D
    out_f32 = 1 if out.dtype == torch.float32 else 0
    _lib.check(lib.hirest_layernorm(_dev(x, torch.float32, "ln.x"), ldx, _opt(row_index, torch.int32, "ln.row_index"),
                                    _dev(gamma, torch.float32, "ln.gamma"), _dev(beta, torch.float32, "ln.beta"),
                                    float(eps), _dev(out, out.dtype, "ln.out"), D, out_f32, rows, D, stream_ptr()),
               "hirest_layernorm")
    return out


@on_tensor_device
def attention(qkv: torch.Tensor, out: torch.Tensor, B: int, N: int, H: int, dh: int, causal: bool,
              scale: Optional[float] = None):
    lib = _lib.load()
    scale = dh ** -0.5 if scale is None else scale
    _lib.check(lib.hirest_attention_bf16(_dev(qkv, torch.bfloat16, "attn.qkv"), _dev(out, torch.bfloat16, "attn.out"),
                                         B, N, H, dh, float(scale), int(bool(causal)), stream_ptr()),
               "hirest_attention_bf16")
    return out


_IN_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}


@on_tensor_device
def patchify(frames: torch.Tensor, patch: int, kpad: int, out: torch.Tensor, mean=None, std=None):
    lib = _lib.load()
    if frames.dtype not in _IN_DTYPES:
        raise RuntimeError(f"patchify: unsupported frame dtype {frames.dtype}")
    code = _IN_DTYPES[frames.dtype]
    B = frames.shape[0]
    S = frames.shape[-1] if code != 2 else frames.shape[1]
    _lib.check(lib.hirest_patchify(_dev(frames, frames.dtype, "patchify.frames"), code, B, S, patch,
                                   _opt(mean, torch.float32, "mean"), _opt(std, torch.float32, "std"),
                                   _dev(out, torch.bfloat16, "patchify.out"), kpad, stream_ptr()), "hirest_patchify")
    return out


@on_tensor_device
def write_cls_rows(x: torch.Tensor, cls: torch.Tensor, pos0: torch.Tensor, B: int, T: int, D: int):
    lib = _lib.load()
    _lib.check(lib.hirest_write_cls_rows(_dev(x, torch.float32, "x"), D, _dev(cls, torch.float32, "cls"),
                                         _dev(pos0, torch.float32, "pos"), B, T, D, stream_ptr()), "hirest_write_cls_rows")
    return x


@on_tensor_device
def embed_tokens(tokens: torch.Tensor, tok_emb: torch.Tensor, pos: torch.Tensor, x: torch.Tensor, eot_row: torch.Tensor):
    lib = _lib.load()
    B, L = tokens.shape
    V, D = tok_emb.shape
    _lib.check(lib.hirest_embed_tokens(_dev(tokens, torch.int64, "tokens"), _dev(tok_emb, torch.float32, "tok_emb"),
                                       _dev(pos, torch.float32, "pos"), _dev(x, torch.float32, "x"),
                                       _dev(eot_row, torch.int32, "eot_row"), B, L, D, V, stream_ptr()), "hirest_embed_tokens")
    return x


@on_tensor_device
def to_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (RNE) on device through the library's cast kernel."""
    lib = _lib.load()
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    n = t.numel()
    if n % 4 != 0:
        raise RuntimeError("to_bf16: element count must be a multiple of 4")
    _lib.check(lib.hirest_f32_to_bf16(_dev(t, torch.float32, "to_bf16.in"), out.data_ptr(), n, stream_ptr()), "hirest_f32_to_bf16")
    return out


@on_tensor_device
def split2(x: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    """[rows, D] fp32 -> [rows, 2D] bf16 in the bf16x3 operand format (hirest_split2_bf16): every 64-column block holds the bf16 hi
    parts of 32 consecutive columns, then their lo parts (lo = bf16(x - hi)).  D % 32 == 0."""
    lib = _lib.load()
    rows, D = x.shape
    out = torch.empty((rows, 2 * D), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.hirest_split2_bf16(_dev(x, torch.float32, "split2.in"), D, out.data_ptr(), 2 * D, rows, D, int(bool(gelu)), stream_ptr()),
               "hirest_split2_bf16")
    return out


@on_tensor_device
def gemm_x3(a2: torch.Tensor, w2: torch.Tensor, bias: Optional[torch.Tensor] = None, resid_out: Optional[torch.Tensor] = None,
            gelu_split: bool = False, stream=None) -> torch.Tensor:
    """fp32 [M, N] = A W^T (+ bias) from split operands a2 [M, 2K], w2 [N, 2K] (ops.split2): HIREST_GEMM_X3.  With `resid_out` (fp32 [M, N])
    the product is added into it (x += ...); with `gelu_split` the result is nn.GELU()(A W^T + bias) as a split operand [M, 2N] bf16
    (HIREST_EPI_BIAS_GELU_SPLIT2: the next layer's A operand, no fp32 round trip)."""
    lib = _lib.load()
    M, K2 = a2.shape
    N = w2.shape[0]
    if gelu_split:
        out = torch.empty((M, 2 * N), dtype=torch.bfloat16, device=a2.device)
        args = _lib.GemmArgs.make(_dev(a2, torch.bfloat16, "gemm_x3.a"), K2, _dev(w2, torch.bfloat16, "gemm_x3.w"), K2,
                                  _opt(bias, torch.float32, "gemm_x3.bias"), out.data_ptr(), 2 * N, M, N, K2, _lib.EPI_BIAS_GELU_SPLIT2, None, 0,
                                  None, None, _lib.GEMM_X3)
        _lib.check(lib.hirest_gemm_bf16(C.byref(args), stream_ptr()), "hirest_gemm_bf16 (x3, gelu + split)")
        return out
    out = resid_out if resid_out is not None else torch.empty((M, N), dtype=torch.float32, device=a2.device)
    epi = _lib.EPI_BIAS_RESID_F32 if resid_out is not None else _lib.EPI_BIAS_F32
    args = _lib.GemmArgs.make(_dev(a2, torch.bfloat16, "gemm_x3.a"), K2, _dev(w2, torch.bfloat16, "gemm_x3.w"), K2,
                              _opt(bias, torch.float32, "gemm_x3.bias"), out.data_ptr(), N, M, N, K2, epi, None, 0, None, None, _lib.GEMM_X3)
    _lib.check(lib.hirest_gemm_bf16(C.byref(args), stream_ptr() if stream is None else stream), "hirest_gemm_bf16 (x3)")
    return out


@on_tensor_device
def pool_l2norm(frame_embeds: torch.Tensor, normalize_frames_first: bool = False) -> torch.Tensor:
    """[V,F,E] f32 -> [V,E]: mean over frames then L2 (inference_video_retrieval.py:283-285)."""
    lib = _lib.load()
    V, F, E = frame_embeds.shape
    out = torch.empty((V, E), dtype=torch.float32, device=frame_embeds.device)
    _lib.check(lib.hirest_pool_l2norm(_dev(frame_embeds, torch.float32, "pool.in"), out.data_ptr(), V, F, E,
                                      int(bool(normalize_frames_first)), stream_ptr()), "hirest_pool_l2norm")
    return out


@on_tensor_device
def similarity(text_n: torch.Tensor, video_n: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    Q, E = text_n.shape
    V = video_n.shape[0]
    out = torch.empty((Q, V), dtype=torch.float32, device=text_n.device)
    _lib.check(lib.hirest_similarity_f32(_dev(text_n, torch.float32, "sim.text"), _dev(video_n, torch.float32, "sim.video"),
                                         out.data_ptr(), Q, V, E, stream_ptr()), "hirest_similarity_f32")
    return out


def gemm_f32_strided(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """alpha * a @ b.T in exact fp32 (hirest_gemm_f32_strided; a [M, K], b [N, K], last dim contiguous)."""
    lib = _lib.load()
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.check(lib.hirest_gemm_f32_strided(_dev(a, torch.float32, "gemm.a"), a.stride(0), 1, _dev(b, torch.float32, "gemm.b"), b.stride(0), 1,
                                           out.data_ptr(), N, M, N, K, float(alpha), stream_ptr()), "hirest_gemm_f32_strided")
    return out


@on_tensor_device
def topk(scores: torch.Tensor, k: int, tie_rank: Optional[torch.Tensor] = None):
    lib = _lib.load()
    Q, V = scores.shape
    idx = torch.empty((Q, k), dtype=torch.int32, device=scores.device)
    val = torch.empty((Q, k), dtype=torch.float32, device=scores.device)
    if V >= 16384:                                   # long rows (beam search over beams * vocab): chunked two-pass selection
        need = lib.hirest_topk_workspace_bytes(Q, V, k)
        ws = torch.empty(need, dtype=torch.uint8, device=scores.device)
        _lib.check(lib.hirest_topk_f32_ws(_dev(scores, torch.float32, "topk.scores"), _opt(tie_rank, torch.int32, "topk.tie_rank"),
                                          Q, V, k, idx.data_ptr(), val.data_ptr(), ws.data_ptr(), need, stream_ptr()),
                   "hirest_topk_f32_ws")
        return val, idx
    _lib.check(lib.hirest_topk_f32(_dev(scores, torch.float32, "topk.scores"), _opt(tie_rank, torch.int32, "topk.tie_rank"),
                                   Q, V, k, idx.data_ptr(), val.data_ptr(), stream_ptr()), "hirest_topk_f32")
    return val, idx



@on_tensor_device
def clip_score(img_rows: torch.Tensor, txt_rows: torch.Tensor, sel) -> torch.Tensor:
    """[C] fp32 CLIPScore (hirest_clip_score): out[c] = mean_j cos(txt_rows[c], img_rows[sel[c, j]]).  img_rows [U, E] and
    txt_rows [C, E] are fp32 or bf16 GPU tensors; sel is an int [C, K] table (CPU or GPU) whose ids are checked against U here."""
    lib = _lib.load()
    if img_rows.dim() != 2 or txt_rows.dim() != 2 or img_rows.shape[1] != txt_rows.shape[1]:
        raise RuntimeError(f"clip_score: expected [U, E] and [C, E] rows, got {tuple(img_rows.shape)} and {tuple(txt_rows.shape)}")
    sel = torch.as_tensor(sel)
    U, E = img_rows.shape
    C = txt_rows.shape[0]
    if sel.dim() != 2 or sel.shape[0] != C or sel.shape[1] < 1:
        raise RuntimeError(f"clip_score: sel must be [C={C}, K>=1], got {tuple(sel.shape)}")
    if sel.numel() and (int(sel.min()) < 0 or int(sel.max()) >= U):
        raise RuntimeError(f"clip_score: row ids must lie in [0, {U})")
    for t, name in ((img_rows, "clip_score.img"), (txt_rows, "clip_score.txt")):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"{name}: expected fp32 or bf16 rows, got {t.dtype}")
    out = torch.empty(C, dtype=torch.float32, device=img_rows.device)
    sel = sel.to(device=img_rows.device, dtype=torch.int32).contiguous()
    _lib.check(lib.hirest_clip_score(_dev(img_rows, img_rows.dtype, "clip_score.img"), _IN_DTYPES[img_rows.dtype], U,
                                     _dev(txt_rows, txt_rows.dtype, "clip_score.txt"), _IN_DTYPES[txt_rows.dtype],
                                     sel.data_ptr(), C, sel.shape[1], E, out.data_ptr(), stream_ptr()), "hirest_clip_score")
    return out

BERTSCORE_MAX_TOKENS = 1024      # HIREST_BERTSCORE_MAX_TOKENS


@on_tensor_device
def bertscore_greedy(states: torch.Tensor, seq_off, tok_weight: torch.Tensor, cand_seq, ref_seq) -> torch.Tensor:
    """[n_pairs, 3] fp32 (P, R, F) of BERTScore's greedy matching (hirest_bertscore_greedy).  states: [tokens, D] fp32 GPU rows of
    the unique sentences (row stride a multiple of 4), sentence s = rows seq_off[s] .. seq_off[s+1]; tok_weight: [tokens] fp32;
    cand_seq / ref_seq: int [n_pairs] sentence ids (an id outside [0, n_seq) gives NaN for its pair).  The int tables may live on
    the CPU or the GPU; a CPU seq_off is checked against the rows here."""
    lib = _lib.load()
    if not isinstance(states, torch.Tensor) or not states.is_cuda or states.dtype != torch.float32 or states.dim() != 2 \
            or (states.numel() and states.stride(1) != 1):
        raise RuntimeError("bertscore_greedy.states: expected a [tokens, D] fp32 GPU tensor with unit column stride")
    rows, D = states.shape
    ld = states.stride(0) if rows > 1 else D
    seq_off, cand_seq, ref_seq = torch.as_tensor(seq_off), torch.as_tensor(cand_seq), torch.as_tensor(ref_seq)
    if seq_off.dim() != 1 or seq_off.numel() < 2 or cand_seq.dim() != 1 or cand_seq.shape != ref_seq.shape:
        raise RuntimeError("bertscore_greedy: seq_off must be [n_seq + 1 >= 2], cand_seq and ref_seq [n_pairs]")
    if not seq_off.is_cuda:
        lens = seq_off[1:] - seq_off[:-1]
        if int(seq_off[0]) < 0 or int(seq_off[-1]) > rows or int(lens.min()) < 1 or int(lens.max()) > BERTSCORE_MAX_TOKENS:
            raise RuntimeError(f"bertscore_greedy.seq_off: sentences of 1 .. {BERTSCORE_MAX_TOKENS} rows inside the {rows} rows")
    if tok_weight.shape != (rows,):
        raise RuntimeError(f"bertscore_greedy.tok_weight: expected [{rows}], got {tuple(tok_weight.shape)}")
    dev = states.device
    seq_off, cand_seq, ref_seq = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (seq_off, cand_seq, ref_seq))
    n_pairs = cand_seq.numel()
    out = torch.empty((n_pairs, 3), dtype=torch.float32, device=dev)
    if n_pairs == 0:
        return out
    _lib.check(lib.hirest_bertscore_greedy(states.data_ptr(), ld, D, seq_off.data_ptr(), seq_off.numel() - 1,
                                           _dev(tok_weight, torch.float32, "bertscore_greedy.tok_weight"), cand_seq.data_ptr(),
                                           ref_seq.data_ptr(), n_pairs, out.data_ptr(), stream_ptr()), "hirest_bertscore_greedy")
    return out


@on_tensor_device
def moment_valid(logits: torch.Tensor, vis_mask: torch.Tensor, moment_mask: torch.Tensor, start_target: torch.Tensor,
                 end_target: torch.Tensor, fill: float = -1e10):
    """(pred [B, 2] int32, loss 0-dim fp32) of moment retrieval's validation pass (hirest_moment_valid_f32): logits [2, B * T] fp32 (start
    head, end head), vis_mask / moment_mask [B, T] int32, start_target / end_target [B] int32 — all on the GPU."""
    lib = _lib.load()
    if vis_mask.dim() != 2 or moment_mask.shape != vis_mask.shape:
        raise ValueError(f"moment_valid: masks must be [B, T], got {tuple(vis_mask.shape)} and {tuple(moment_mask.shape)}")
    B, T = vis_mask.shape
    if B < 1 or T < 1 or tuple(logits.shape) != (2, B * T) or tuple(start_target.shape) != (B,) or tuple(end_target.shape) != (B,):
        raise ValueError(f"moment_valid: expected logits [2, {B * T}] and targets [{B}], got {tuple(logits.shape)}, "
                         f"{tuple(start_target.shape)}, {tuple(end_target.shape)}")
    pred = torch.empty((B, 2), dtype=torch.int32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    _lib.check(lib.hirest_moment_valid_f32(_dev(logits, torch.float32, "moment_valid.logits"), _dev(vis_mask, torch.int32, "moment_valid.vis_mask"),
                                           _dev(moment_mask, torch.int32, "moment_valid.moment_mask"),
                                           _dev(start_target, torch.int32, "moment_valid.start_target"),
                                           _dev(end_target, torch.int32, "moment_valid.end_target"), B, T, float(fill), pred.data_ptr(),
                                           loss.data_ptr(), stream_ptr()), "hirest_moment_valid_f32")
    return pred, loss


@on_tensor_device
def lm_head_ce(h: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, target: torch.Tensor, n_valid: Optional[int] = None):
    """(nll [R] fp32, loss 0-dim fp32): CrossEntropyLoss(ignore_index=-1) of h @ w.T + bias without a stored logit
    (hirest_lm_head_ce_f32).  h [R, 768], w [V, 768], bias [V] fp32, target [R] int32 on the GPU; n_valid = the number of rows with
    target >= 0 (default R: every row counts), known to the caller from its host copy of the targets."""
    lib = _lib.load()
    if h.dim() != 2 or w.dim() != 2 or h.shape[0] < 1 or w.shape[0] < 1 or h.shape[1] != w.shape[1]:
        raise ValueError(f"lm_head_ce: expected h [R, K] and w [V, K], got {tuple(h.shape)} and {tuple(w.shape)}")
    R, K = h.shape
    V = w.shape[0]
    if tuple(bias.shape) != (V,) or tuple(target.shape) != (R,):
        raise ValueError(f"lm_head_ce: expected bias [{V}] and target [{R}], got {tuple(bias.shape)} and {tuple(target.shape)}")
    n_valid = R if n_valid is None else int(n_valid)
    if n_valid < 0 or n_valid > R:
        raise ValueError(f"lm_head_ce: n_valid must lie in [0, {R}], got {n_valid}")
    need = lib.hirest_lm_head_ce_workspace_bytes(R, V)
    ws = torch.empty(need, dtype=torch.uint8, device=h.device)
    nll = torch.empty((R,), dtype=torch.float32, device=h.device)
    loss = torch.empty((), dtype=torch.float32, device=h.device)
    _lib.check(lib.hirest_lm_head_ce_f32(_dev(h, torch.float32, "lm_head_ce.h"), K, _dev(w, torch.float32, "lm_head_ce.w"), K,
                                         _dev(bias, torch.float32, "lm_head_ce.bias"), _dev(target, torch.int32, "lm_head_ce.target"),
                                         R, V, K, n_valid, nll.data_ptr(), loss.data_ptr(), ws.data_ptr(), need, stream_ptr()),
               "hirest_lm_head_ce_f32")
    return nll, loss


def to_device(t: torch.Tensor, device) -> torch.Tensor:
    """t.to(device) that does not stall the host when it need not: a pinned CPU tensor (what DataLoader(pin_memory=True) delivers:
    hirest_dataset.py:614,624) is copied asynchronously on the current stream — the kernels that read it are behind it on the same
    stream — everything else as t.to(device).  As with any non_blocking copy, the source must not be overwritten before the copy has
    run (DataLoader hands out fresh pinned tensors per batch; a caller that refills one pinned buffer in place must synchronise first)."""
    if t.device.type == "cpu" and t.is_pinned():
        return t.to(device, non_blocking=True)
    return t.to(device)


_STREAM_WS = {}
_STREAM_WS_RETIRED = []


def stream_workspace(device, nbytes: int, tag=0, stream: Optional[int] = None):
    """Scratch that a C call uses on ONE stream (hirest_gemm_f32_ws, the split form of few-tile fp32 GEMMs; the bf16x3 encoder): one
    buffer per (device, tag, stream), so two streams never share scratch (`tag` tells users on one stream apart — 0: the fp32 GEMMs,
    1: the training step's side stream; `stream` = the raw stream pointer the call is enqueued on, default the current torch
    stream).  Grown geometrically on demand; an outgrown buffer is RETIRED, not freed: torch's caching allocator only orders a
    block's reuse against the stream it was allocated on, and the calls still in flight on this key's stream may be reading
    it — the retired blocks (their sizes sum to less than the live buffer) stay referenced for the life of the process.
    Returns (pointer, bytes) — (None, 0) when the problem wants none."""
    if nbytes <= 0:
        return None, 0
    key = (device.type, device.index, tag, int(stream) if stream is not None else stream_ptr())
    buf = _STREAM_WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _STREAM_WS_RETIRED.append(buf)
        buf = torch.empty(max(int(nbytes), 2 * (buf.numel() if buf is not None else 0), 32 << 20), dtype=torch.uint8, device=device)
        _STREAM_WS[key] = buf
    return buf.data_ptr(), buf.numel()
