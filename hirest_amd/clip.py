"""Drop-in for the reference's vendored OpenAI-CLIP module (/root/reference/EVA_clip/clip.py + model.py),
ViT variants only (the ResNet visual towers of model.py:10-163 are never instantiated by any HiREST caller).

    model, preprocess = clip.load("/path/to/ViT-B-32.pt", device="cuda")     # clip.py:94 (state-dict or JIT archive)
    model = clip.build_model(state_dict)                                       # model.py:434-471 (dims inferred)
    tokens = clip.tokenize(["a photo of a cat"])                               # clip.py:196

Behavioural notes that callers rely on (and that the parity tests pin against the reference):
* the vendored ``VisionTransformer.forward`` drops the CLS token and returns ``ln_post(patch tokens) @ proj``:
  ``encode_image`` -> ``[B, grid^2, embed_dim]`` (model.py:269-273; SURVEY hazard H4), not a CLS embedding;
* QuickGELU activations, ``ln_pre`` before the stack, conv1 without bias, LayerNorm eps 1e-5;
* ``encode_text`` = EOT-row gather @ text_projection (model.py:343-356).
Compute: the same gfx950 kernels as hirest_amd.eva_clip (bf16 MFMA GEMMs, fp32 statistics).  No download
support (no network): ``load`` needs a local file.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Union

import torch
from torch import nn

from . import _lib, ops
from .eva_clip import (OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, _NO_FOLD, _RESBLOCK, TextTower, _Leaf, _Tower, _linear, _norm,
                       _precision_scope, image_transform)
from .tokenizer import tokenize  # noqa: F401  (clip.tokenize)

__all__ = ["available_models", "load", "tokenize", "build_model", "CLIP"]


def available_models() -> List[str]:
    """clip.py:89-91 lists downloadable names; offline there are none — pass a checkpoint path to ``load``."""
    return []


class OpenAIVisionTower(_Tower):
    """model.py:216-273, parameter names identical (conv1, class_embedding, positional_embedding, ln_pre,
    transformer.resblocks.N.*, ln_post, proj)."""
    _what = "CLIP vision tower"
    _FIELDS = (("patch_w", "patch", "conv1.weight"), ("patch_b", None, None),                     # conv1 has no bias (model.py:220)
               ("cls", "f32", "class_embedding"), ("pos", "f32", "positional_embedding"),
               ("norm_g", "f32", "ln_post.weight"), ("norm_b", "f32", "ln_post.bias"), ("head_w", "wT", "proj"), ("head_b", None, None),
               ("image_mean", "const", "image_mean"), ("image_std", "const", "image_std"),
               ("ln_pre_g", "f32", "ln_pre.weight"), ("ln_pre_b", "f32", "ln_pre.bias"))
    _TABLES = {"bf16": (_lib.VisionTower, _FIELDS, _lib.BlockWeights, _RESBLOCK + _NO_FOLD),
               "fp32": (_lib.VisionTowerF32, _FIELDS, _lib.BlockWeightsF32, _RESBLOCK)}
    image_mean, image_std = OPENAI_DATASET_MEAN, OPENAI_DATASET_STD

    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        self.input_resolution, self.patch_size, self.width, self.layers, self.heads = input_resolution, patch_size, width, layers, heads
        self.output_dim = output_dim
        self.grid = input_resolution // patch_size
        self.num_tokens = self.grid ** 2 + 1
        D = width
        self.conv1 = _Leaf(weight=(D, 3, patch_size, patch_size))
        self.class_embedding = nn.Parameter(torch.zeros(D))
        self.positional_embedding = nn.Parameter(torch.zeros(self.num_tokens, D))
        self.ln_pre = _norm(D)
        self.transformer = nn.Module()
        blocks = []
        for _ in range(layers):
            b = nn.Module()
            b.attn = _Leaf(in_proj_weight=(3 * D, D), in_proj_bias=(3 * D,))
            b.attn.out_proj = _linear(D, D)
            b.ln_1, b.ln_2 = _norm(D), _norm(D)
            b.mlp = nn.Module()
            b.mlp.c_fc, b.mlp.c_proj = _linear(4 * D, D), _linear(D, 4 * D)
            blocks.append(b)
        self.transformer.resblocks = nn.ModuleList(blocks)
        # 'bf16' (default: the MFMA towers) | 'fp32' (exact-fp32 kernels of csrc/tower_f32.hip with its QuickGELU epilogue, ln_pre and
        # all-token head: the reference's own arithmetic, so cosines land within 1e-5 of it and its top-k ids are reproduced);
        # CLIP.set_precision / clip.load(..., precision=) / HIREST_PRECISION select it
        self.precision = "bf16"
        self.pip_head = False          # True: return the CLS embedding like the pip `clip` package (clip.load(..., pip_head=True))
        self.ln_post = _norm(D)
        self.proj = nn.Parameter(torch.zeros(D, output_dim))
        self.max_frames_per_call = 2048

    def _blocks(self):
        return self.transformer.resblocks

    def _scalars(self):
        D, P = self.width, self.patch_size
        return dict(image_size=self.input_resolution, patch=P, width=D, heads=self.heads, head_dim=D // self.heads, mlp_dim=4 * D,
                    layers=self.layers, embed_dim=self.output_dim, kpad=(3 * P * P + 63) // 64 * 64,
                    act=1, ln_eps=1e-5,       # QuickGELU (model.py:175), nn.LayerNorm default eps
                    out_all_tokens=1)         # ln_pre; ln_post + proj on every token (model.py:229-273)

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
            x = x.float()
        f32 = self.precision != "bf16"
        desc = C.byref(self._prepared_for("fp32" if f32 else "bf16", x.device)["desc"])
        lib = _lib.load()
        x = x.contiguous()
        B, T, E = x.shape[0], self.num_tokens, self.output_dim
        out = torch.empty((B, T, E), dtype=torch.float32, device=x.device)
        if B == 0:
            return out[:, 0, :] if self.pip_head else out[:, 1:, :]
        code = ops._IN_DTYPES[x.dtype]

        def call(s, n, ws):
            if f32:
                _lib.check(lib.hirest_vision_forward_f32(desc, x[s:s + n].data_ptr(), code, n, out[s:s + n].data_ptr(), ws.data_ptr(),
                                                         ws.numel(), ops.stream_ptr()), "hirest_vision_forward_f32")
            else:
                _lib.check(lib.hirest_vision_forward(desc, x[s:s + n].data_ptr(), code, n, out[s:s + n].data_ptr(), ws.data_ptr(),
                                                     ws.numel(), 0, ops.stream_ptr()), "hirest_vision_forward")
        wsb = lib.hirest_vision_workspace_bytes_f32 if f32 else lib.hirest_vision_workspace_bytes
        limit = self.max_frames_per_call if f32 else self._frames_limit(self.max_frames_per_call, T)
        self._run_calls(B, limit, False, lambda n: wsb(desc, n), call, x.device)
        if self.pip_head:
            # the pip `clip` package's head (openai/CLIP @ a9b1bf5, model.py VisionTransformer.forward: ln_post(x[:, 0, :]) @ proj):
            # LayerNorm and projection act per token, so it is row 0 of what the kernel computed for every token
            return out[:, 0, :]
        return out[:, 1:, :]            # w/o cls token (model.py:269)


class CLIP(nn.Module):
    """model.py:277-406 (ViT visual only)."""

    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size,
                 context_length, vocab_size, transformer_width, transformer_heads, transformer_layers):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("ModifiedResNet visual towers are not used by HiREST and not implemented")
        self.context_length = context_length
        self.visual = OpenAIVisionTower(image_resolution, vision_patch_size, vision_width, vision_layers,
                                        vision_width // 64, embed_dim)
        # the text tower's parameters sit at the top level in the reference; reuse TextTower and re-export them
        t = TextTower(vocab_size, transformer_width, transformer_layers, transformer_heads, context_length, embed_dim,
                      quick_gelu=True)
        object.__setattr__(self, "_text", t)          # not a registered submodule: names below are the real ones
        self.transformer = t.transformer
        self.token_embedding = t.token_embedding
        self.positional_embedding = t.positional_embedding
        self.ln_final = t.ln_final
        self.text_projection = t.text_projection
        self.logit_scale = t.logit_scale
        self.vocab_size = vocab_size

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._text.invalidate()
        self._text._workspace = None
        return r

    def _load_from_state_dict(self, *a, **k):
        self._text.invalidate()
        return super()._load_from_state_dict(*a, **k)

    def set_precision(self, precision: str):
        """'bf16' = the bf16 MFMA towers (default); 'fp32' = both towers in exact fp32 (the reference's own arithmetic: model.py runs in
        fp32 on CPU, clip.py:136-138): cosines within 1e-5 of the reference, its top-k ids reproduced; 'bf16x3' is accepted and runs the
        fp32 kernels (ViT-B/32 is 4.4 GFLOP per frame: the exact path is cheap, no split-operand variant is built for it)."""
        if precision not in ("bf16", "fp32", "bf16x3"):
            raise ValueError(f"precision must be one of ('bf16', 'fp32', 'bf16x3'), got {precision!r}")
        p = "bf16" if precision == "bf16" else "fp32"
        self.visual.precision = p
        self._text.precision = p
        return self

    def precision_scope(self, visual: str = None, text: str = None):
        """``with model.precision_scope(visual='fp32'):`` runs the block with the named towers at another precision and puts back what
        they had, also when the block raises.  Names as in ``set_precision``: 'bf16x3' runs the fp32 kernels."""
        for precision in (visual, text):
            if precision not in (None, "bf16", "fp32", "bf16x3"):
                raise ValueError(f"precision must be one of ('bf16', 'fp32', 'bf16x3'), got {precision!r}")
        to = {None: None, "bf16": "bf16", "fp32": "fp32", "bf16x3": "fp32"}
        return _precision_scope(((self.visual, to[visual]), (self._text, to[text])))

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image):
        return self.visual(image)

    def encode_text(self, text):
        return self._text(text)

    def forward(self, image, text):
        """model.py:358-372: cosine logits scaled by exp(logit_scale)."""
        img = self.encode_image(image)
        txt = self.encode_text(text)
        # F.normalize = the pooling kernel with one row per "video"; logits = exp(logit_scale) * img_n txt_n^T on the fp32 MFMA GEMM
        img = ops.pool_l2norm(img.float().unsqueeze(1).contiguous())
        txt = ops.pool_l2norm(txt.float().unsqueeze(1).contiguous())
        logits_per_image = ops.gemm_f32_strided(img, txt, float(torch.exp(self.logit_scale.detach().float().cpu())))
        return logits_per_image, logits_per_image.transpose(-1, -2)


def build_model(state_dict: Dict[str, torch.Tensor]) -> CLIP:
    """model.py:434-471: infer every dimension from the checkpoint, load strictly, return in eval mode."""
    if "visual.proj" not in state_dict:
        raise NotImplementedError("only ViT CLIP checkpoints are supported (ModifiedResNet is unused by HiREST)")
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
    grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    image_resolution = vision_patch_size * grid_size
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    model = CLIP(embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_heads, transformer_layers)
    sd = {k: v for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return model.eval()


def load(name: str, device: Union[str, torch.device] = "cuda", jit: bool = False, download_root: str = None, pip_head: bool = False,
         precision: str = "bf16"):
    """clip.py:94-193 for local checkpoints: a JIT archive or a plain state dict -> (model, preprocess).

    ``pip_head=True`` gives the model of the *pip* ``clip`` package (openai/CLIP @ a9b1bf5, requirements.txt:25) that the reference's
    ``'clip'`` retrieval branch imports (inference_video_retrieval.py:11,169; hirest_dataset.py:84): same weights, same tower, but
    ``encode_image`` returns the CLS embedding ``ln_post(x[:, 0]) @ proj`` -> [B, embed_dim] instead of the vendored copy's projected
    patch tokens.  That package is not part of the reference tree, so this head is checked against the oracle's restatement of its
    published forward and against transformers' CLIPModel on the same weights (tests/test_gpu_clip_score.py)."""
    if not os.path.isfile(name):
        raise RuntimeError(f"Model {name} not found; available models = {available_models()}")
    try:
        state_dict = torch.jit.load(name, map_location="cpu").eval().state_dict()
    except RuntimeError:
        state_dict = torch.load(name, map_location="cpu")
    model = build_model(state_dict).to(device)
    # precision: this argument, unless HIREST_PRECISION (the opt-in for unmodified reference callers, as in eva_clip.create_model) is set
    env = os.environ.get("HIREST_PRECISION", "").strip().lower()
    model.set_precision(env or precision)
    model.visual.pip_head = bool(pip_head)
    return model, image_transform(model.visual.input_resolution)
