"""Drop-in for the inference side of the reference's joint model, ``MomentModel.test_step``
(/root/reference/modeling.py:141-153): moment retrieval (modeling.py:272-310) and iterative moment
segmentation (modeling.py:353-474) over precomputed 1-fps EVA-CLIP frame features + ASR features.

Same constructor arguments, batch dict keys (hirest_dataset.py:409-531: ``tasks``, ``vis_feats``,
``vis_mask``, ``moment_mask``, ``asr_feats``, ``clip_text_ids``, ``moment_bound_frames``) and result dict
(``prediction`` / ``raw_predictions``) as the reference; the parameter tree reproduces the reference's
state-dict keys (``clip_g_map``, ``asr_enc_layer.{0,1}``, ``temporal_embed.{0,2}``, ``mask_embed``,
``boundary_embed``, ``{start,end,segment}_predictor.0``, ``clip4cap_model.visual.*`` ...), so a reference
``BEST.pth`` loads with ``load_state_dict(strict=False)`` exactly as ``trainer_base.py:128-147`` does.

All math runs in the fp32 kernels of csrc/joint.hip (+ the LayerNorm kernel).  What differs from the
reference is where time goes: the 20 segmentation iterations run back to back on the device —
masks, softmax, arg-max, threshold walk and step list are device state, with ONE device->host copy at the
end instead of B x 20 ``.cpu().tolist()`` syncs — and the loop-invariant part of the fusion is hoisted.
Step captioning (modeling.py:556-632): trim_feats, the same fusion/encoder on 20 frames, then beam search over the
2-layer decoder — decoder math in the fp32 kernels, beam bookkeeping on the host as in the reference.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from copy import deepcopy
from typing import List

import numpy as np
import torch
from torch import nn

from . import _lib, caption_search, ops

def _p(*shape):
    return nn.Parameter(torch.zeros(*shape))


class _Lin(nn.Module):
    def __init__(self, out_f, in_f):
        super().__init__()
        self.weight, self.bias = _p(out_f, in_f), _p(out_f)


class _LN(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight, self.bias = _p(d), _p(d)


class _Emb(nn.Module):
    def __init__(self, n, d):
        super().__init__()
        self.weight = _p(n, d)


def _seq(**mods):
    m = nn.Module()
    for k, v in mods.items():
        m.add_module(k, v)
    return m


_BUILD_CLIP = "build"      # default of MomentModel(clip_model=...): construct the CLIP as the reference's __init__ does


class MomentModel(nn.Module):
    """modeling.py:18-129 (inference subset).

    ``MomentModel(n_frames, asr_dim, args)`` — the reference's three-argument call (run.py:52-56) — builds and freezes its
    own text encoder exactly as modeling.py:115-123 does: ``build_eva_model_and_transforms("EVA_CLIP_g_14",
    pretrained="./pretrained_weights/eva_clip_psz14.pt")``, ``.float()``, ``.eval()``, ``freeze_clip()``; a missing
    checkpoint raises ``FileNotFoundError`` there as it does in the reference.  The towers stay on the host until the
    model is moved; their kernel-ready device buffers are prepared on the first ``encode_text`` after ``.to(cuda)``.
    ``args.clip_model_name`` / ``args.clip_pretrained`` (not reference options; default to the two literals above)
    redirect the build, e.g. to a synthetic checkpoint offline.
    Pass ``clip_model=<EVA_CLIP>`` to share an already built encoder, or ``clip_model=None`` for a model that is fed
    ``batch['text_feat']`` (the commented-out alternative at modeling.py:284) and owns no CLIP."""

    def __init__(self, n_frames=-1, asr_dim=-1, args=None, clip_model=_BUILD_CLIP, max_position_embeddings=2048):
        super().__init__()
        self.args, self.n_frames, self.asr_dim = args, n_frames, asr_dim
        self.use_asr = asr_dim > 0
        E, H = 512, 768
        if self.use_asr:
            self.asr_enc_layer = _seq(**{"0": _LN(asr_dim), "1": _Lin(E, asr_dim)})
        self.temporal_embed = _seq(**{"0": _Lin(E, 1), "2": _Lin(E, E)})
        self.mask_embed, self.boundary_embed = _Emb(2, E), _Emb(2, E)
        self.start_predictor = _seq(**{"0": _Lin(1, H)})
        self.end_predictor = _seq(**{"0": _Lin(1, H)})
        self.segment_predictor = _seq(**{"0": _Lin(1, H)})
        vis = nn.Module()
        vis.embeddings = _seq(word_embeddings=_Lin(H, E), position_embeddings=_Emb(max_position_embeddings, H), LayerNorm=_LN(H))
        layers = []
        for _ in range(getattr(args, "visual_num_hidden_layers", 2) if args is not None else 2):
            lay = nn.Module()
            lay.attention = nn.Module()
            lay.attention.self = _seq(query=_Lin(H, H), key=_Lin(H, H), value=_Lin(H, H))
            lay.attention.output = _seq(dense=_Lin(H, H), LayerNorm=_LN(H))
            lay.intermediate = _seq(dense=_Lin(4 * H, H))
            lay.output = _seq(dense=_Lin(H, 4 * H), LayerNorm=_LN(H))
            layers.append(lay)
        vis.encoder = nn.Module()
        vis.encoder.layer = nn.ModuleList(layers)
        self.clip4cap_model = nn.Module()
        self.clip4cap_model.visual = vis
        self.clip4cap_model.normalize_video = _seq(visual_norm2d=_LN(E))
        # caption decoder (clip4caption/modules/module_decoder.py:279-406); LM head tied to the input embedding
        vocab = 30522
        dec = nn.Module()
        dec.embeddings = _seq(word_embeddings=_Emb(vocab, H), position_embeddings=_Emb(512, H), LayerNorm=_LN(H))
        dlayers = []
        for _ in range(getattr(args, "decoder_num_hidden_layers", 2) if args is not None else 2):
            lay = nn.Module()
            for nm in ("slf_attn", "enc_attn"):
                att = nn.Module()
                att.att = _seq(query=_Lin(H, H), key=_Lin(H, H), value=_Lin(H, H))
                att.output = _seq(dense=_Lin(H, H), LayerNorm=_LN(H))
                lay.add_module(nm, att)
            lay.intermediate = _seq(dense=_Lin(4 * H, H))
            lay.output = _seq(dense=_Lin(H, 4 * H), LayerNorm=_LN(H))
            dlayers.append(lay)
        dec.decoder = nn.Module()
        dec.decoder.layer = nn.ModuleList(dlayers)
        pred = nn.Module()
        pred.bias = _p(vocab)
        pred.transform = _seq(dense=_Lin(H, H), LayerNorm=_LN(H))
        pred.decoder = nn.Module()
        pred.decoder.weight = dec.embeddings.word_embeddings.weight       # tied (module_decoder.py:171-176)
        dec.classifier = nn.Module()
        dec.classifier.cls = nn.Module()
        dec.classifier.cls.predictions = pred
        self.clip4cap_model.decoder = dec
        self.tokenizer_vocab = None      # optional id -> token list (BERT vocab is not available offline)
        self.clip_g_map, self.clip_g_map_text = _Lin(E, 1024), _Lin(E, 1024)
        if isinstance(clip_model, str) and clip_model == _BUILD_CLIP:
            from .eva_clip import build_eva_model_and_transforms                 # modeling.py:114-123
            clip_model, self.clip_preprocess = build_eva_model_and_transforms(
                getattr(args, "clip_model_name", None) or "EVA_CLIP_g_14",
                pretrained=getattr(args, "clip_pretrained", None) or "./pretrained_weights/eva_clip_psz14.pt")
            print("Loaded EVA CLIP G")
            clip_model = clip_model.float()
            clip_model.eval()
        self.clip_model = clip_model
        self.freeze_clip()
        self.heads = 12
        self.caption_kv_cache = True   # step captioning keeps the decoder's self-attention K / V per beam (False: full-prefix recompute)
        self._cache = None
        # 'fp32' (default: the reference's own arithmetic, modeling.py:120 / run.py without --fp16) or 'bf16x3': the encoder's linear layers on
        # split operands (csrc/joint_x3.hip) — the counterpart of the reference's reduced-precision mode (torch.cuda.amp.autocast() under
        # --fp16, run.py:549-551), at 16 significand bits per product so that indices / boundaries / token ids stay the fp32 run's
        self.precision = "fp32"
        if os.environ.get("HIREST_JOINT_PRECISION"):
            self.set_precision(os.environ["HIREST_JOINT_PRECISION"])

    def set_precision(self, precision: str):
        """'fp32': every product exact fp32 (v_mfma_f32_*_f32).  'bf16x3': the VisualModel encoder's weight GEMMs (moment retrieval, the 20
        segmentation passes, the captioning encoder pass) as three bf16 MFMAs on hi + lo splits of both fp32 operands; attention, LayerNorm,
        GELU, residuals, fusion, heads and the caption decoder stay fp32."""
        if precision not in ("fp32", "bf16x3"):
            raise ValueError(f"MomentModel precision must be 'fp32' or 'bf16x3', got {precision!r}")
        self.precision = precision
        return self

    # ------------------------------------------------------------------ nn.Module plumbing
    def _apply(self, fn, *a, **k):
        self._cache = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._cache = None
        return super()._load_from_state_dict(*a, **k)

    def freeze_clip(self):   # modeling.py:126-129
        if self.clip_model is not None:
            for p in self.clip_model.parameters():
                p.requires_grad = False
            self.clip_model.eval()

    def _w(self):
        """fp32 contiguous device views + fused QKV weights, built once per parameter version.

        Most entries are views of the parameters and follow in-place optimizer updates; the fused / padded tensors
        (QKV concatenations, padded LM head, head biases, any non-fp32 parameter) are COPIES, so the cache remembers the
        ``_version`` counters of their sources and is rebuilt when one of them has moved (run.py:328-336 validates after
        every epoch of in-place AdamW steps)."""
        if self._cache is not None:
            if sum(p._version for p in self._cache["copied"]) == self._cache["copied_version"]:
                return self._cache
            self._cache = None
        dev = self.clip_g_map.weight.device
        if dev.type != "cuda":
            raise RuntimeError("hirest_amd.MomentModel runs on MI355X only (no CPU fallback); move the model to a GPU")
        f = lambda t: t.detach().float().contiguous()
        c = {"dev": dev}
        copied = []
        for name, prm in self.named_parameters():
            if not name.startswith("clip_model."):
                c[name] = f(prm)
                if c[name].data_ptr() != prm.data_ptr():
                    copied.append(prm)
        for i, lay in enumerate(self.clip4cap_model.visual.encoder.layer):
            s = lay.attention.self
            c[f"qkv_w.{i}"] = torch.cat([f(s.query.weight), f(s.key.weight), f(s.value.weight)], 0).contiguous()
            c[f"qkv_b.{i}"] = torch.cat([f(s.query.bias), f(s.key.bias), f(s.value.bias)], 0).contiguous()
        for i, lay in enumerate(self.clip4cap_model.decoder.decoder.layer):
            sa, ea = lay.slf_attn.att, lay.enc_attn.att
            c[f"dec_qkv_w.{i}"] = torch.cat([f(sa.query.weight), f(sa.key.weight), f(sa.value.weight)], 0).contiguous()
            c[f"dec_qkv_b.{i}"] = torch.cat([f(sa.query.bias), f(sa.key.bias), f(sa.value.bias)], 0).contiguous()
            c[f"dec_kv_w.{i}"] = torch.cat([f(ea.key.weight), f(ea.value.weight)], 0).contiguous()
            c[f"dec_kv_b.{i}"] = torch.cat([f(ea.key.bias), f(ea.value.bias)], 0).contiguous()
        # LM head: vocab padded to a multiple of 4 rows for the GEMM's 4-wide epilogue; pad logits are -3e38 so they
        # vanish in the log-softmax and can never enter the top-k
        we = f(self.clip4cap_model.decoder.embeddings.word_embeddings.weight)
        vb = f(self.clip4cap_model.decoder.classifier.cls.predictions.bias)
        padn = (-we.shape[0]) % 4
        c["lm_w"] = torch.cat([we, torch.zeros((padn, we.shape[1]), device=dev)], 0).contiguous() if padn else we
        c["lm_b"] = torch.cat([vb, torch.full((padn,), -3.0e38, device=dev)]).contiguous() if padn else vb
        # descriptor of the C-side decoder step (csrc/caption.hip): device pointers into the tensors above
        Dp = "clip4cap_model.decoder."
        nl = len(self.clip4cap_model.decoder.decoder.layer)
        layers = (_lib.CaptionLayer * nl)()
        for i in range(nl):
            p = Dp + f"decoder.layer.{i}."
            layers[i] = _lib.CaptionLayer(*[c[k].data_ptr() for k in (
                f"dec_qkv_w.{i}", f"dec_qkv_b.{i}", p + "slf_attn.output.dense.weight", p + "slf_attn.output.dense.bias",
                p + "slf_attn.output.LayerNorm.weight", p + "slf_attn.output.LayerNorm.bias",
                p + "enc_attn.att.query.weight", p + "enc_attn.att.query.bias", p + "enc_attn.output.dense.weight",
                p + "enc_attn.output.dense.bias", p + "enc_attn.output.LayerNorm.weight", p + "enc_attn.output.LayerNorm.bias",
                p + "intermediate.dense.weight", p + "intermediate.dense.bias", p + "output.dense.weight", p + "output.dense.bias",
                p + "output.LayerNorm.weight", p + "output.LayerNorm.bias")])
        cp = Dp + "classifier.cls.predictions."
        c["dec_layers"] = layers
        c["dec_desc"] = _lib.CaptionDecoder(
            nl, self.heads, 768, c[Dp + "decoder.layer.0.intermediate.dense.weight"].shape[0], c["lm_w"].shape[0],
            c[Dp + "embeddings.position_embeddings.weight"].shape[0],
            c[Dp + "embeddings.word_embeddings.weight"].data_ptr(), c[Dp + "embeddings.position_embeddings.weight"].data_ptr(),
            c[Dp + "embeddings.LayerNorm.weight"].data_ptr(), c[Dp + "embeddings.LayerNorm.bias"].data_ptr(), layers,
            c[cp + "transform.dense.weight"].data_ptr(), c[cp + "transform.dense.bias"].data_ptr(),
            c[cp + "transform.LayerNorm.weight"].data_ptr(), c[cp + "transform.LayerNorm.bias"].data_ptr(),
            c["lm_w"].data_ptr(), c["lm_b"].data_ptr(), None)
        c["head_bias"] = torch.cat([f(getattr(m, "0").bias) for m in
                                    (self.start_predictor, self.end_predictor, self.segment_predictor)]).contiguous()
        for lay in self.clip4cap_model.visual.encoder.layer:
            copied += [q for m in (lay.attention.self.query, lay.attention.self.key, lay.attention.self.value) for q in m.parameters()]
        for lay in self.clip4cap_model.decoder.decoder.layer:
            copied += [q for a in (lay.slf_attn.att, lay.enc_attn.att) for m in (a.query, a.key, a.value) for q in m.parameters()]
        copied += [self.clip4cap_model.decoder.embeddings.word_embeddings.weight, self.clip4cap_model.decoder.classifier.cls.predictions.bias]
        copied += [getattr(m, "0").bias for m in (self.start_predictor, self.end_predictor, self.segment_predictor)]
        c["copied"] = copied
        c["copied_version"] = sum(p._version for p in copied)
        self._cache = c
        return c

    def _x3(self):
        """Split-operand weights + the C-side descriptor of the encoder (hirest_joint_encoder_x3), built once per parameter version: every
        [N, K] fp32 weight becomes [N, 2K] bf16 (hirest_split2_bf16: per 32 k, hi | lo).  Lives in the weight cache, so an optimizer step or a
        load_state_dict rebuilds it with the rest."""
        c, lib = self._w(), _lib.load()
        if "x3" in c:
            return c["x3"]
        dev = c["dev"]

        def split(w):
            w = w.contiguous()
            out = torch.empty((w.shape[0], 2 * w.shape[1]), dtype=torch.bfloat16, device=dev)
            _lib.check(lib.hirest_split2_bf16(w.data_ptr(), w.shape[1], out.data_ptr(), 2 * w.shape[1], w.shape[0], w.shape[1], 0,
                                              ops.stream_ptr()), "hirest_split2_bf16")
            return out
        V = "clip4cap_model.visual."
        nl = len(self.clip4cap_model.visual.encoder.layer)
        keep, layers = [], (_lib.JointLayerX3 * nl)()
        for i in range(nl):
            p = V + f"encoder.layer.{i}."
            w2 = [split(c[f"qkv_w.{i}"]), split(c[p + "attention.output.dense.weight"]), split(c[p + "intermediate.dense.weight"]),
                  split(c[p + "output.dense.weight"])]
            keep += w2
            layers[i] = _lib.JointLayerX3(
                w2[0].data_ptr(), c[f"qkv_b.{i}"].data_ptr(), w2[1].data_ptr(), c[p + "attention.output.dense.bias"].data_ptr(),
                c[p + "attention.output.LayerNorm.weight"].data_ptr(), c[p + "attention.output.LayerNorm.bias"].data_ptr(),
                w2[2].data_ptr(), c[p + "intermediate.dense.bias"].data_ptr(), w2[3].data_ptr(), c[p + "output.dense.bias"].data_ptr(),
                c[p + "output.LayerNorm.weight"].data_ptr(), c[p + "output.LayerNorm.bias"].data_ptr())
        emb = split(c[V + "embeddings.word_embeddings.weight"])
        keep.append(emb)
        H = c[V + "embeddings.LayerNorm.weight"].shape[0]
        pos = c[V + "embeddings.position_embeddings.weight"]
        desc = _lib.JointEncoderX3(C.sizeof(_lib.JointEncoderX3), nl, self.heads, H, c[V + "encoder.layer.0.intermediate.dense.weight"].shape[0],
                                   c[V + "embeddings.word_embeddings.weight"].shape[1], pos.shape[0], 1e-12, -10000.0,
                                   emb.data_ptr(), c[V + "embeddings.word_embeddings.bias"].data_ptr(), pos.data_ptr(),
                                   c[V + "embeddings.LayerNorm.weight"].data_ptr(), c[V + "embeddings.LayerNorm.bias"].data_ptr(), layers)
        # the caption decoder's descriptor with the LM head's weights in the split format as well (csrc/caption.hip takes them at >= 64 rows)
        lm2 = split(c["lm_w"])
        keep.append(lm2)
        d0 = c["dec_desc"]
        dec = _lib.CaptionDecoder(*[getattr(d0, n) for n, _ in _lib.CaptionDecoder._fields_[:-1]], lm2.data_ptr())
        c["x3"] = {"desc": desc, "layers": layers, "keep": keep, "width": H, "dec_desc": dec}
        return c["x3"]

    def _dec_desc(self):
        """The C-side decoder descriptor of the current precision ('bf16x3': with the split LM head)."""
        return self._x3()["dec_desc"] if self.precision == "bf16x3" else self._w()["dec_desc"]

    def _encoder_x3(self, f2d: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """VisualModel.forward on split operands: ONE C call (csrc/joint_x3.hip) issues the embeddings and both blocks."""
        x3, lib = self._x3(), _lib.load()
        need = lib.hirest_joint_encoder_x3_workspace_bytes(C.byref(x3["desc"]), B, T)
        if need == 0:
            raise RuntimeError("hirest_joint_encoder_x3: unsupported encoder shape")
        st = ops.stream_ptr()
        ws, wsb = ops.stream_workspace(f2d.device, need, "encoder_x3", st)     # per stream: caption_batches runs this on several at once
        out = torch.empty((B * T, x3["width"]), dtype=torch.float32, device=f2d.device)
        _lib.check(lib.hirest_joint_encoder_x3_forward(C.byref(x3["desc"]), f2d.data_ptr(), B, T, out.data_ptr(), ws, wsb, st),
                   "hirest_joint_encoder_x3_forward")
        return out

    # ------------------------------------------------------------------ kernels
    @staticmethod
    def _gemm(a, w, bias, out=None, resid=None, periodic=None, period=0, act=0):
        lib = _lib.load()
        M, K = a.shape
        N = w.shape[0]
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=a.device)
        ws, wsb = ops.stream_workspace(a.device, lib.hirest_gemm_f32_workspace_bytes(M, N, K))
        _lib.check(lib.hirest_gemm_f32_ws(a.data_ptr(), K, w.data_ptr(), w.shape[1], bias.data_ptr() if bias is not None else None,
                                          resid.data_ptr() if resid is not None else None, N,
                                          periodic.data_ptr() if periodic is not None else None, period,
                                          out.data_ptr(), N, M, N, K, act, ws, wsb, ops.stream_ptr()), "hirest_gemm_f32_ws")
        return out

    @staticmethod
    def _ln(x, w, b, eps):
        out = torch.empty_like(x)
        return ops.layernorm(x, w, b, eps, out)

    def _encoder(self, f2d: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """VisualModel.forward (module_visual.py:396-424): embeddings + 2 post-LN layers, fp32."""
        c, lib = self._w(), _lib.load()
        V = "clip4cap_model.visual."
        x = self._gemm(f2d, c[V + "embeddings.word_embeddings.weight"], c[V + "embeddings.word_embeddings.bias"],
                       periodic=c[V + "embeddings.position_embeddings.weight"], period=T)
        x = self._ln(x, c[V + "embeddings.LayerNorm.weight"], c[V + "embeddings.LayerNorm.bias"], 1e-12)
        D = x.shape[1]
        for i in range(len(self.clip4cap_model.visual.encoder.layer)):
            p = V + f"encoder.layer.{i}."
            qkv = self._gemm(x, c[f"qkv_w.{i}"], c[f"qkv_b.{i}"])
            ctx = torch.empty_like(x)
            _lib.check(lib.hirest_attention_f32(qkv.data_ptr(), ctx.data_ptr(), B, T, self.heads, D // self.heads,
                                                (D // self.heads) ** -0.5, -10000.0, ops.stream_ptr()), "hirest_attention_f32")
            a = self._gemm(ctx, c[p + "attention.output.dense.weight"], c[p + "attention.output.dense.bias"], resid=x)
            a = self._ln(a, c[p + "attention.output.LayerNorm.weight"], c[p + "attention.output.LayerNorm.bias"], 1e-12)
            h = self._gemm(a, c[p + "intermediate.dense.weight"], c[p + "intermediate.dense.bias"], act=1)
            y = self._gemm(h, c[p + "output.dense.weight"], c[p + "output.dense.bias"], resid=a)
            x = self._ln(y, c[p + "output.LayerNorm.weight"], c[p + "output.LayerNorm.bias"], 1e-12)
        return x

    def _fusion_base(self, vis, text, asr, vis_mask) -> torch.Tensor:
        """Loop-invariant part of foward_moment_shared (modeling.py:158-195): v*t + asr + temporal."""
        c, lib = self._w(), _lib.load()
        B, T, _ = vis.shape
        E = 512
        v = self._gemm(vis.reshape(B * T, -1), c["clip_g_map.weight"], c["clip_g_map.bias"])
        v = self._ln(v, c["clip4cap_model.normalize_video.visual_norm2d.weight"],
                     c["clip4cap_model.normalize_video.visual_norm2d.bias"], 1e-12)
        tproj = self._gemm(text, c["clip_g_map_text.weight"], c["clip_g_map_text.bias"])
        if self.use_asr:
            a = self._ln(asr.reshape(B * T, -1).contiguous(), c["asr_enc_layer.0.weight"], c["asr_enc_layer.0.bias"], 1e-5)
            a = self._gemm(a, c["asr_enc_layer.1.weight"], c["asr_enc_layer.1.bias"])
        else:
            a = torch.zeros((B * T, E), dtype=torch.float32, device=vis.device)
        n_valid = vis_mask.sum(dim=-1).to(torch.int32).contiguous()
        tin = torch.empty((B * T, E), dtype=torch.float32, device=vis.device)
        _lib.check(lib.hirest_joint_time_features(n_valid.data_ptr(), c["temporal_embed.0.weight"].data_ptr(),
                                                  c["temporal_embed.0.bias"].data_ptr(), tin.data_ptr(), B, T, E,
                                                  ops.stream_ptr()), "hirest_joint_time_features")
        temporal = self._gemm(tin, c["temporal_embed.2.weight"], c["temporal_embed.2.bias"])
        base = torch.empty((B * T, E), dtype=torch.float32, device=vis.device)
        _lib.check(lib.hirest_joint_base(v.data_ptr(), tproj.data_ptr(), a.data_ptr(), temporal.data_ptr(), base.data_ptr(),
                                         B, T, E, ops.stream_ptr()), "hirest_joint_base")
        return base

    def _features(self, base, moment_mask_i32, boundary_mask_i32, B, T) -> torch.Tensor:
        c, lib = self._w(), _lib.load()
        f = torch.empty_like(base)
        _lib.check(lib.hirest_joint_mask_add(base.data_ptr(), moment_mask_i32.data_ptr(),
                                             boundary_mask_i32.data_ptr() if boundary_mask_i32 is not None else None,
                                             c["mask_embed.weight"].data_ptr(), c["boundary_embed.weight"].data_ptr(),
                                             f.data_ptr(), B * T, 512, ops.stream_ptr()), "hirest_joint_mask_add")
        return self._encoder_x3(f, B, T) if self.precision == "bf16x3" else self._encoder(f, B, T)

    def _heads(self, feats, which: List[str]) -> torch.Tensor:
        c, lib = self._w(), _lib.load()
        rows, D = feats.shape
        names = {"start": ("start_predictor.0.weight", 0), "end": ("end_predictor.0.weight", 1), "segment": ("segment_predictor.0.weight", 2)}
        ws = [c[names[w][0]] for w in which]
        bkey = "head_bias3." + ".".join(which)             # (lives in the weight cache: rebuilt with it when a parameter changes)
        bias3 = c.get(bkey)
        if bias3 is None:
            bias3 = torch.stack([c["head_bias"][names[w][1]] for w in which]).contiguous()
            bias3 = c[bkey] = torch.cat([bias3, torch.zeros(3 - len(which), device=bias3.device)]).contiguous()
        logits = torch.empty((len(which), rows), dtype=torch.float32, device=feats.device)
        _lib.check(lib.hirest_linear_heads(feats.data_ptr(), rows, D, len(which), ws[0].data_ptr(),
                                           ws[1].data_ptr() if len(ws) > 1 else None, ws[2].data_ptr() if len(ws) > 2 else None,
                                           bias3.data_ptr(), logits.data_ptr(), ops.stream_ptr()), "hirest_linear_heads")
        return logits

    # ------------------------------------------------------------------ reference interface
    def _text_feat(self, batch, device):
        if "text_feat" in batch:
            return ops.to_device(batch["text_feat"], device).float().contiguous()
        if self.clip_model is None:
            raise RuntimeError("MomentModel needs clip_model (encode_text) or batch['text_feat']")
        return self.clip_model.encode_text(batch["clip_text_ids"].to(device)).float().contiguous()

    def test_step(self, batch, **kwargs):
        task = batch["tasks"][0]
        dev = self.clip_g_map.weight.device
        # kernels launch on the model's device, whatever the process's current device is (the reference never calls
        # set_device in single-process runs: run.py:61-65)
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            if task == "moment_retrieval":
                return self.test_moment_retrieval(batch, **kwargs)
            elif task == "moment_segmentation":
                return self.test_moment_segmentation(batch, **kwargs)
            elif task == "step_captioning":
                return self.test_step_captioning(batch, **kwargs)
            else:
                raise NotImplementedError

    def train_step(self, batch):
        """modeling.py:130-140: ``{'loss': tensor}``; ``loss.backward()`` fills ``param.grad`` through the kernels of
        csrc/train.hip (hirest_amd/train.py), for all three tasks."""
        from . import train
        task = batch["tasks"][0]
        dev = self.clip_g_map.weight.device
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            if task == "moment_retrieval":
                return train.train_moment_retrieval(self, batch)
            elif task == "moment_segmentation":
                return train.train_moment_segmentation(self, batch)
            elif task == "step_captioning":
                return train.train_step_captioning(self, batch)
            else:
                raise NotImplementedError

    # ------------------------------------------------------------------ validation pass (run.py:546-571)
    @torch.no_grad()
    def valid_step(self, batch, **gen_kwargs):
        """What ``Trainer.predict(has_target=True)`` takes from a batch (run.py:548-571: ``train_step`` under ``eval()`` and ``no_grad``, then
        ``test_step``), from ONE forward: ``{'loss': 0-dim fp32 device tensor, 'prediction': ...}`` plus whatever else ``test_step`` returns.
        The loss is the reference's training loss with dropout off, whatever ``self.training`` says; the prediction is ``test_step``'s,
        bit for bit.  The text feature, the fusion and the encoder run once, on the inference path (``set_precision`` applies).

        moment_retrieval: both results from the same head logits in one launch (hirest_moment_valid_f32).  step_captioning: one encoder
        pass and one cross-attention K / V projection feed a teacher-forced decoder pass over the target prefix — only the rows with a
        target go through the LM head, whose logits are never stored (hirest_lm_head_ce_f32) — and the beam search (``search=False``:
        the loss alone; hirest_amd.predict then captions several batches with one search).
        moment_segmentation: the teacher-forced loss reads ``prev_boundary_mask`` inputs the iterative inference never sees, so with
        targets in the batch it is ``train_step``'s loss beside ``test_step``'s prediction; without them, ``test_step``'s result alone."""
        from . import train
        task = batch["tasks"][0]
        dev = self.clip_g_map.weight.device
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            if task == "moment_retrieval":
                return self._valid_moment_retrieval(batch)
            elif task == "moment_segmentation":
                res = self.test_moment_segmentation(batch, **gen_kwargs)
                if "moment_segmentation_target" in batch and "prev_boundary_mask" in batch:
                    res = {"loss": train.eval_loss(self, batch), **res}
                return res
            elif task == "step_captioning":
                return self._valid_step_captioning(batch, **gen_kwargs)
            else:
                raise NotImplementedError

    def _valid_moment_retrieval(self, batch):
        dev = self._w()["dev"]
        i32 = lambda t: ops.to_device(t, dev).to(torch.int32).contiguous()
        vis, vmask, mmask = ops.to_device(batch["vis_feats"], dev).float().contiguous(), i32(batch["vis_mask"]), i32(batch["moment_mask"])
        asr = ops.to_device(batch["asr_feats"], dev).float().contiguous() if self.use_asr else None
        B, T = vmask.shape
        base = self._fusion_base(vis, self._text_feat(batch, dev), asr, vmask)
        logits = self._heads(self._features(base, mmask, None, B, T), ["start", "end"])              # [2, B * T]
        pred, loss = ops.moment_valid(logits, vmask, mmask, i32(batch["moment_retrieval_start_target"]).reshape(-1),
                                      i32(batch["moment_retrieval_end_target"]).reshape(-1))
        return {"loss": loss, "prediction": pred.cpu().tolist()}

    @staticmethod
    def _caption_targets(batch):
        """The teacher-forcing triples of ``batch['target_text']`` (fields 5, 6, 7 of the reference's 9-tuples) as [B, max_words] int64
        host arrays: decoder input ids, decoder mask, output ids (-1 = ignored)."""
        row = lambda f: np.asarray(f, dtype=np.int64).reshape(-1)
        tt = batch["target_text"]
        return tuple(np.stack([row(t[k]) for t in tt]) for k in (5, 6, 7))

    def _caption_loss(self, enc_kv_all, input_ids, output_ids):
        """CrossEntropyLoss(ignore_index=-1) of the teacher-forced decoder (modeling.py:516-521) on the K / V rows of the inference
        encoder.  The prefix is cut to the longest valid length of the batch (a later position cannot reach an earlier one through the
        causal mask), the rows with a target are gathered, and only those go through the LM-head transform and hirest_lm_head_ce_f32.
        input_ids / output_ids: [B, L] int64 host arrays.  Without any target the loss is 0, as train_step's is."""
        c = self._w()
        dev = c["dev"]
        b_idx, p_idx = np.nonzero(output_ids >= 0)
        if b_idx.size == 0:
            return torch.zeros((), dtype=torch.float32, device=dev)
        L = int(p_idx.max()) + 1
        ids = torch.from_numpy(np.ascontiguousarray(input_ids[:, :L])).to(dev)
        rows = torch.from_numpy(b_idx.astype(np.int64) * L + p_idx).to(dev)
        target = torch.from_numpy(output_ids[b_idx, p_idx].astype(np.int32)).to(dev)
        hidden = caption_search.decoder_hidden(self, ids, enc_kv_all).index_select(0, rows)
        return ops.lm_head_ce(caption_search.lm_head_transform(self, hidden), c["lm_w"], c["lm_b"], target)[1]

    @staticmethod
    def _causal_mask_is_exact(decoder_mask, output_ids) -> bool:
        """The reference masks padded keys as well as future keys (module_decoder.py:388-397).  Where every position with a target has
        no padded key at or before it — the loader's masks: ones, then zeros — the causal penalty alone gives its scores."""
        L = decoder_mask.shape[1]
        last = np.where(output_ids >= 0, np.arange(L)[None, :], -1).max(axis=1)                     # last position with a target, -1: none
        first_pad = np.where(decoder_mask == 0, np.arange(L)[None, :], L).min(axis=1)               # first padded key, L: none
        return bool((first_pad > last).all())

    def _valid_step_captioning(self, batch, num_beams=5, return_ids=False, search=True, **kwargs):
        """`search=False`: the loss alone (hirest_amd.predict captions several loader batches with ONE beam search afterwards)."""
        from . import train
        dev = self._w()["dev"]
        input_ids, decoder_mask, output_ids = self._caption_targets(batch)
        enc_kv_all = self._caption_encoder_kv(*self._caption_inputs(batch, dev))
        if self._causal_mask_is_exact(decoder_mask, output_ids):
            loss = self._caption_loss(enc_kv_all, input_ids, output_ids)
        else:                                   # a padded key in front of a target: the training forward applies the full mask
            loss = train.eval_loss(self, batch)
        if not search:
            return {"loss": loss}
        res = caption_search.search(self, enc_kv_all, num_beams, self._caption_limits()[1], return_ids, kwargs.get("graph_slot"))
        return {"loss": loss, **res}

    @torch.no_grad()
    def forward_moment_retrieval(self, video_feats, text_feat, video_mask=None, moment_mask=None, asr_feats=None):
        """modeling.py:212-224: returns {'start_logits','end_logits'} [B,T] (fp32, unmasked)."""
        B, T, _ = video_feats.shape
        video_feats = video_feats.float().contiguous()
        if video_mask is None:
            video_mask = torch.ones((B, T), dtype=torch.long, device=video_feats.device)
        base = self._fusion_base(video_feats, text_feat, asr_feats.float().contiguous() if asr_feats is not None else None, video_mask)
        feats = self._features(base, moment_mask.to(torch.int32).contiguous(), None, B, T)
        lg = self._heads(feats, ["start", "end"])
        return {"start_logits": lg[0].reshape(B, T), "end_logits": lg[1].reshape(B, T), "feats": feats.reshape(B, T, -1)}

    @torch.no_grad()
    def test_moment_retrieval(self, batch, **kwargs):
        lib = _lib.load()
        dev = self._w()["dev"]
        vis, vmask, mmask = batch["vis_feats"].to(dev), batch["vis_mask"].to(dev), batch["moment_mask"].to(dev)
        asr = batch["asr_feats"].to(dev) if self.use_asr else None
        out = self.forward_moment_retrieval(vis, self._text_feat(batch, dev), vmask, mmask, asr)
        B, T = vmask.shape
        m32 = vmask.to(torch.int32).contiguous()
        pred = torch.empty((2, B), dtype=torch.int32, device=dev)
        for i, k in enumerate(("start_logits", "end_logits")):
            _lib.check(lib.hirest_masked_argmax(out[k].contiguous().data_ptr(), m32.data_ptr(), -1e10, B, T,
                                                pred[i].data_ptr(), ops.stream_ptr()), "hirest_masked_argmax")
        return {"prediction": pred.t().cpu().tolist()}

    @torch.no_grad()
    def test_moment_segmentation(self, batch, threshold=0.15, return_trace=False, **kwargs):
        lib = _lib.load()
        dev = self._w()["dev"]
        vis, vmask = batch["vis_feats"].to(dev).float().contiguous(), batch["vis_mask"].to(dev)
        asr = batch["asr_feats"].to(dev).float().contiguous() if self.use_asr else None
        text = self._text_feat(batch, dev)
        B, T = vmask.shape
        starts = batch["moment_bound_frames"][:, 0].tolist()
        lasts = batch["moment_bound_frames"][:, 1].tolist()
        mm = torch.zeros((B, T), dtype=torch.int32)
        bm = torch.zeros((B, T), dtype=torch.int32)
        for b in range(B):
            mm[b, starts[b]:lasts[b] + 1] = 1
            bm[b, starts[b]] = 1
        mm, bm = mm.to(dev), bm.to(dev)
        thr = float(getattr(self.args, "moment_segmentation_difference_threshold", 0.5)) if self.args is not None else 0.5
        iters = int(getattr(self.args, "moment_segmentation_max_iterations", 20)) if self.args is not None else 20
        steps = torch.zeros((B, iters, 2), dtype=torch.int32, device=dev)
        nsteps = torch.zeros((B,), dtype=torch.int32, device=dev)
        base = self._fusion_base(vis, text, asr, vmask)
        first_logits = None
        for it in range(iters):                                   # no host sync inside the loop
            feats = self._features(base, mm, bm, B, T)
            logits = self._heads(feats, ["segment"])[0].contiguous()
            if it == 0 and return_trace:
                first_logits = logits.reshape(B, T).clone()
            _lib.check(lib.hirest_segmentation_step(logits.data_ptr(), mm.data_ptr(), bm.data_ptr(), B, T, thr,
                                                    steps.data_ptr(), nsteps.data_ptr(), iters, None, ops.stream_ptr()),
                       "hirest_segmentation_step")
        steps_h, n_h = steps.cpu().tolist(), nsteps.cpu().tolist()    # the only device->host copy
        preds = []
        for b in range(B):                                         # modeling.py:435-463, pure Python ints
            sp = [[starts[b], starts[b]]] + [list(s) for s in steps_h[b][:n_h[b]]] + [[lasts[b], lasts[b]]]
            sp.sort(key=lambda x: x[0])
            flat = [v for s in sp for v in s]
            while flat[-1] > lasts[b]:
                flat.pop(-1)
            temp = sorted(set(flat))
            keep, cur = [temp[0]], temp[0]
            for i in range(1, len(temp) - 1):
                if temp[i] - cur >= 5:
                    keep.append(temp[i])
                    cur = temp[i]
            preds.append(keep)
        res = {"raw_predictions": deepcopy(preds), "prediction": preds}
        if return_trace:
            res["first_logits"] = first_logits
        return res


    # ------------------------------------------------------------------ step captioning (modeling.py:529-632)
    @staticmethod
    def _trim_index(mask_row: List[int], max_frames: int) -> List[int]:
        """Row indices selected by trim_feats (modeling.py:529-554) for one sample; -1 = zero row."""
        sel = [i for i, m in enumerate(mask_row) if m == 1]
        N = len(sel)
        if N == 0:
            return [-1] * max_frames
        if max_frames < N:
            return sel[:max_frames]
        idx = []
        for j in range(N):
            idx += [sel[j]] * (((j + 1) * max_frames) // N - (j * max_frames) // N)
        return idx + [-1] * (max_frames - len(idx))

    def _trim_rows(self, moment_mask: torch.Tensor, max_frames: int, device):
        """The row-index table of trim_feats for a batch, on `device`: flat row numbers b * T + t into the [B * T, D] feature matrix,
        [B * max_frames] long, and — only when some sample selects fewer than max_frames rows — a [B * max_frames, 1] 0 / 1 column
        that zeroes the missing ones (else None).  Host index arithmetic on the mask as the collate function delivers it (a CPU
        tensor: no device round trip; a device tensor costs one copy back, not one per sample), uploaded once and shared by the
        visual and the ASR features."""
        idx = self._trim_index_table(moment_mask.cpu(), max_frames)              # [B, max_frames] int64, -1 = zero row
        B, T = moment_mask.shape
        flat = torch.from_numpy(np.maximum(idx, 0) + np.arange(B, dtype=np.int64)[:, None] * T).reshape(-1)
        keep = None
        if (idx < 0).any():
            keep = torch.from_numpy((idx >= 0).astype(np.float32).reshape(-1, 1)).to(device)
        return flat.to(device), keep

    @staticmethod
    def _host_moment_mask(batch) -> torch.Tensor:
        """``batch['moment_mask']`` for the host index arithmetic of trim_feats: a batch built on the device (hirest_amd.dataset)
        carries a CPU copy in ``batch.host``, so the mask never travels back; any other batch gives the entry itself."""
        host = getattr(batch, "host", None)
        if host and "moment_mask" in host:
            return host["moment_mask"]
        return batch["moment_mask"]

    @staticmethod
    def _trim_index_table(mask: torch.Tensor, max_frames: int) -> "np.ndarray":
        """_trim_index for every row of a [B, T] CPU mask at once (the per-sample list walk cost 0.5 ms of host time in front of a B = 32
        captioning batch, with the GPU idle): output position p of a sample with N <= max_frames selected frames takes selected frame
        ceil((p + 1) N / max_frames) - 1 — the closed form of the reference's repeat counts (j + 1) F // N - j F // N (modeling.py:529-554)."""
        m = mask.numpy() == 1
        B, T = m.shape
        F = int(max_frames)
        N = m.sum(axis=1).astype(np.int64)                                       # selected frames per sample
        sel = np.argsort(~m, axis=1, kind="stable")                              # selected frame numbers first, in order
        p = np.arange(F, dtype=np.int64)[None, :]
        Nc = np.maximum(N, 1)[:, None]
        j = np.where(N[:, None] > F, p, ((p + 1) * Nc + F - 1) // F - 1)         # more frames than slots: the first F; else repeats
        idx = np.take_along_axis(sel, np.minimum(j, T - 1), axis=1).astype(np.int64)
        idx[N == 0] = -1
        return idx

    def _trim(self, feats: torch.Tensor, moment_mask, max_frames: int, idx=None) -> torch.Tensor:
        if idx is None:
            idx = self._trim_rows(moment_mask, max_frames, feats.device)
        flat, keep = idx
        B, T, D = feats.shape
        out = feats.reshape(B * T, D).index_select(0, flat)                    # pure data movement
        if keep is not None:
            out = out * keep
        return out.reshape(B, max_frames, D)

    # the search itself lives in hirest_amd/caption_search.py; its switches stay here
    CAPTION_GRAPH_CHUNK = 8           # words per captured hipGraph of the search replayed by caption_batches (caption_search.capture)
    CAPTION_ROWS_IN_FLIGHT = 160      # beam rows of one merged search (caption_batches): 32 videos x 5 beams, the reference's default eval batch
    caption_fused_tail = True         # log-softmax, top-k and beam bookkeeping inside the word step's C call; False: separate kernels
    caption_device_readout = True     # the best hypothesis of every sample walked back on the device (hirest_beam_backtrack); False: on the host (BeamState)

    @torch.no_grad()
    def test_step_captioning(self, batch, num_beams=5, return_ids=False, **kwargs):
        """modeling.py:556-632.  Returns {'prediction': [str]} (token strings joined like the reference; ids are
        printed as decimal strings when no BERT vocab is attached via ``tokenizer_vocab``)."""
        return self._caption_trimmed(*self._caption_inputs(batch, self._w()["dev"]), num_beams, return_ids, **kwargs)

    def _caption_limits(self):
        """(max_frames, max_words) of step captioning: args.max_frames_step_captioning / args.max_words, the reference's defaults without args."""
        return int(getattr(self.args, "max_frames_step_captioning", 20)), int(getattr(self.args, "max_words", 48))

    def _caption_inputs(self, batch, dev):
        """trim_feats (modeling.py:529-554) of one loader batch: (vis [B, max_frames, D], asr [B, max_frames, Da] or None, text [B, 1024])."""
        max_frames = self._caption_limits()[0]
        rows = self._trim_rows(self._host_moment_mask(batch), max_frames, dev)
        v = self._trim(batch["vis_feats"].to(dev).float(), None, max_frames, idx=rows)
        a = self._trim(batch["asr_feats"].to(dev).float(), None, max_frames, idx=rows) if self.use_asr else None
        return v, a, self._text_feat(batch, dev)

    def _caption_encoder_kv(self, v, a, text):
        """The fusion and the encoder on the trimmed frames, then the cross-attention K / V of every decoder layer ([B, max_frames, 1536]
        each): loop invariant for the beam search, and shared with the teacher-forced loss by valid_step."""
        c, (B, max_frames) = self._w(), v.shape[:2]
        ones = torch.ones((B, max_frames), dtype=torch.long, device=c["dev"])
        base = self._fusion_base(v, text, a, ones)
        enc = self._features(base, ones.to(torch.int32).contiguous(), None, B, max_frames)          # [B*F, 768]
        return [self._gemm(enc, c[f"dec_kv_w.{i}"], c[f"dec_kv_b.{i}"]).reshape(B, max_frames, -1)
                for i in range(len(self.clip4cap_model.decoder.decoder.layer))]

    def _caption_trimmed(self, v, a, text, num_beams, return_ids, **kwargs):
        """test_step_captioning behind trim_feats: v [B, max_frames, D] (a [B, max_frames, Da] or None) already trimmed, text [B, 1024]."""
        return caption_search.search(self, self._caption_encoder_kv(v, a, text), num_beams, self._caption_limits()[1], return_ids,
                                     kwargs.get("graph_slot"))

    @torch.no_grad()
    def caption_batches(self, batches, num_beams=5, streams=1, return_ids=False, graphs=True, merge=True, rows_in_flight=None):
        """Step captioning over a LIST of loader batches (the evaluation loop of run.py:328-336 / modeling.py:556-632 calls
        test_step once per batch).

        merge=True (default): consecutive batches are captioned by ONE beam search over the union of their beam rows, up to
        `rows_in_flight` rows (default CAPTION_ROWS_IN_FLIGHT = 160 = the reference's default --eval_batch_size 32 at beam 5,
        args.py:27) — a word's 162 MB of decoder weights are then streamed once for all of them instead of once per batch; each
        sample keeps its own done flag and the search ends when all have emitted [SEP].  The merged groups (if more than one) then go
        through the machinery below, up to `streams` in flight (default 1: a search of ~150 rows is matrix-pipe time, a second one beside
        it gains nothing — 1697 vs 1616 captions/s for twelve batches of 5 at beam 5).  merge=False: every loader batch is its own search (round 4).

        Up to `streams` searches in flight, each on its own HIP stream and host thread.

        Why: one batch of 5 videos x 5 beams is 25 rows — a word step is ~20 dependent kernels of a few microseconds each, bound by
        launch and memory latency, not by the 162 MB of weights it streams: the GPU is mostly idle.  Independent batches
        fill those gaps; only the LM head (HBM-bound, all CUs) serialises.  Every call owns its buffers (workspace, K / V cache, beam
        state, pinned done table), the weight cache is read-only, and every kernel is batch-invariant, so each batch's result is
        exactly what ``test_step`` returns for it alone.  Returns the per-batch result dicts in order."""
        return caption_search.caption_batches(self, batches, num_beams, streams, return_ids, graphs, merge, rows_in_flight)

    @torch.no_grad()
    def end_to_end(self, batch, num_beams=5, return_ids=False):
        """The reference's ``run.py --end_to_end`` (run.py:383-490) for one moment-retrieval batch: retrieval, segmentation of the
        retrieved moment and a caption per predicted step, chained on the device (hirest_amd/cascade.py, csrc/cascade.hip).

        ``batch`` is what the moment-retrieval loader delivers (``vis_feats``, ``vis_mask``, an all-ones ``moment_mask``, ``asr_feats``
        when the model uses ASR, ``text_feat`` or ``clip_text_ids``) plus ``video_duration`` [B] and, where the number of bins differs
        per sample (the loader's ``n_model_frames = -1``: one frame per second), ``n_frames`` [B]; without it the model's ``n_frames``
        is used (<= 0: one frame per second of each duration).  The text feature is computed once for all three stages and
        ``set_precision`` applies as it does to ``test_step``.

        Returns a dict of per-sample lists: ``moment_frames`` [start, end] (the arg-max frames), ``bounds`` [start_s, end_s]
        (run.py:731-734), ``boundary_frames`` (the segmentation's ``prediction``), ``step_bounds`` [[s0, s1], [s1, s2], ...] in seconds
        (run.py:766-776) and ``captions`` (one string per step; the token-id lists with ``return_ids``).

        Deviation from the reference: a sample whose segmentation yields fewer than two boundaries has no step; it gets
        ``step_bounds = []`` and ``captions = []`` here, where the reference's captioning dataset raises IndexError on the empty
        step list (hirest_dataset.py:279 under --end_to_end)."""
        from . import cascade
        return cascade.run_end_to_end(self, [batch], num_beams=num_beams, return_ids=return_ids)[0]

    def _caption_texts(self, hyps, return_ids):
        vocab = self.tokenizer_vocab
        if vocab is None:                                    # ids printed as decimal strings: no '[SEP]' / '[PAD]' / '##' to handle
            texts = [" ".join(map(str, h)) for h in hyps]
        else:
            texts = []
            for h in hyps:
                toks = [vocab[i] for i in h]
                if "[SEP]" in toks:
                    toks = toks[:toks.index("[SEP]")]
                if "[PAD]" in toks:
                    toks = toks[:toks.index("[PAD]")]
                texts.append(" ".join(toks).replace(" ##", "").strip("##").strip())
        res = {"prediction": texts}
        if return_ids:
            res["token_ids"] = hyps
        return res
