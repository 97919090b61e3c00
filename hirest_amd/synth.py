"""Deterministic synthetic weights / inputs (no pretrained checkpoints exist offline).

Every value is a pure function of (seed, tensor name, flat index): a splitmix64 hash of
the index, top 24 bits -> uniform in [-1, 1) -> scaled.  Only integer ops and exact
float64 multiplies are used, so the generated tensors are bit-identical on every
machine / numpy / torch build (``torch.manual_seed`` gives no such guarantee).  The
golden-vector script, the CPU oracle, the parity tests and ``bench.py`` all draw their
weights from here, so "same inputs" is true by construction on both sides of a
comparison.

The state-dict *key names and shapes* are the reference's checkpoint schema
(``eva_clip_psz14.pt``: /root/reference/EVA_clip/eva_model.py:177-315,
vit_model.py:248-310; OpenAI CLIP: EVA_clip/model.py:216-331), so the same dict loads
into the reference modules via ``load_state_dict`` and into this package's towers.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

_M64 = (1 << 64) - 1


def _fnv1a64(s: str) -> int:
    h = 0xCBF29CE484222325
    for b in s.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & _M64
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def uniform_pm1(name: str, n: int, seed: int) -> np.ndarray:
    """n float64 values, uniform on the 2^-23 grid in [-1, 1)."""
    base = np.uint64((_fnv1a64(name) ^ ((seed * 0x9E3779B97F4A7C15) & _M64)) & _M64)
    out = np.empty(n, dtype=np.float64)
    step = 1 << 22
    for s in range(0, n, step):
        e = min(n, s + step)
        with np.errstate(over="ignore"):
            idx = np.arange(s, e, dtype=np.uint64) + base
        z = _splitmix64(idx)
        out[s:e] = (z >> np.uint64(40)).astype(np.float64) * (2.0 / (1 << 24)) - 1.0
    return out


def tensor(name: str, shape, std: float, seed: int, mean: float = 0.0) -> torch.Tensor:
    """fp32 tensor with the given std (uniform distribution of matching variance).  Same values as
    ``(uniform_pm1(...) * (std * sqrt(3)) + mean).astype(float32)``, produced chunk by chunk straight into the fp32
    result (a 1 B-parameter checkpoint never exists in float64)."""
    n = int(np.prod(shape)) if len(shape) else 1
    base = np.uint64((_fnv1a64(name) ^ ((seed * 0x9E3779B97F4A7C15) & _M64)) & _M64)
    v = np.empty(n, dtype=np.float32)
    scale = std * math.sqrt(3.0)
    step = 1 << 20
    for s in range(0, n, step):
        e = min(n, s + step)
        with np.errstate(over="ignore"):
            idx = np.arange(s, e, dtype=np.uint64) + base
        u = (_splitmix64(idx) >> np.uint64(40)).astype(np.float64) * (2.0 / (1 << 24)) - 1.0
        v[s:e] = u * scale + mean
    return torch.from_numpy(v.reshape(tuple(shape)))


def frames(name: str, shape, seed: int) -> torch.Tensor:
    """Synthetic already-normalised frames: unit-variance values (N(0,1)-like)."""
    return tensor(name, shape, 1.0, seed)


def rgb_frames(name: str, shape, seed: int) -> np.ndarray:
    """Synthetic decoded video frames, uint8 [..., H, W, 3]: 8x8-pixel flat blocks (hard edges, so the bicubic
    resampler's negative lobes overshoot and the 0/255 clamps are exercised) with per-pixel noise on half of them."""
    shape = tuple(int(v) for v in shape)
    *lead, h, w, c = shape
    nb = int(np.prod(lead)) if lead else 1
    fine = ((uniform_pm1(name + ".fine", nb * h * w * c, seed) + 1.0) * 128.0).astype(np.int64).clip(0, 255)
    fine = fine.reshape(nb, h, w, c)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    coarse = ((uniform_pm1(name + ".coarse", nb * bh * bw * c, seed) + 1.0) * 128.0).astype(np.int64).clip(0, 255)
    coarse = np.repeat(np.repeat(coarse.reshape(nb, bh, bw, c), 8, axis=1), 8, axis=2)[:, :h, :w]
    pick = uniform_pm1(name + ".pick", nb * bh * bw, seed).reshape(nb, bh, bw, 1) > 0.0
    pick = np.repeat(np.repeat(pick, 8, axis=1), 8, axis=2)[:, :h, :w]
    out = np.where(pick, coarse, (coarse + fine) // 2).astype(np.uint8)
    return out.reshape(shape)


def tokens(name: str, batch: int, seed: int, context_length: int = 77,
           vocab_size: int = 49408) -> torch.Tensor:
    """Synthetic CLIP token rows: [SOT] ids... [EOT] 0-padding (clip.py:196-232 layout).

    EOT (vocab-1) is the largest id in each row, which is what ``text.argmax(-1)``
    (eva_model.py:243) relies on.
    """
    sot, eot = vocab_size - 2, vocab_size - 1
    u = uniform_pm1(name, batch * context_length, seed).reshape(batch, context_length)
    lens = 3 + ((uniform_pm1(name + ".len", batch, seed) + 1.0) * 0.5 * 20).astype(np.int64)
    ids = ((u + 1.0) * 0.5 * (vocab_size - 1000)).astype(np.int64) + 300
    out = np.zeros((batch, context_length), dtype=np.int64)
    for b in range(batch):
        n = int(lens[b])
        out[b, 0] = sot
        out[b, 1:1 + n] = ids[b, :n]
        out[b, 1 + n] = eot
    return torch.from_numpy(out)


# ----------------------------------------------------------------------------------
# EVA-CLIP (vision: BEiT-style ViT; text: open_clip-style transformer)
# ----------------------------------------------------------------------------------

EVA_CLIP_G_14 = {  # /root/reference/EVA_clip/model_configs/EVA_CLIP_g_14.json
    "embed_dim": 1024,
    "vision_cfg": {"image_size": 224, "layers": 40, "width": 1408, "head_width": 88,
                   "mlp_ratio": 4.3637, "patch_size": 14, "drop_path_rate": 0.4},
    "text_cfg": {"context_length": 77, "vocab_size": 49408, "width": 768, "heads": 12,
                 "layers": 12},
}

# A small config with the awkward dimensions of the real one (head_dim 88, 257 tokens,
# mlp_ratio that truncates) for fast CPU parity checks.  Widths are multiples of 64 (the
# GEMM's K granule): 704 = 8 heads x 88.
EVA_CLIP_TINY = {
    "embed_dim": 64,
    "vision_cfg": {"image_size": 224, "layers": 2, "width": 704, "head_width": 88,
                   "mlp_ratio": 4.3637, "patch_size": 14, "drop_path_rate": 0.0},
    "text_cfg": {"context_length": 77, "vocab_size": 49408, "width": 128, "heads": 2,
                 "layers": 2},
}


def eva_vision_shapes(cfg: dict) -> Dict[str, Tuple[int, ...]]:
    v = cfg["vision_cfg"]
    D, P, L = v["width"], v["patch_size"], v["layers"]
    N = (v["image_size"] // P) ** 2 + 1
    Dm = int(D * v["mlp_ratio"])  # vit_model.py:166
    E = cfg["embed_dim"]
    s = {"visual.cls_token": (1, 1, D), "visual.pos_embed": (1, N, D),
         "visual.patch_embed.proj.weight": (D, 3, P, P), "visual.patch_embed.proj.bias": (D,)}
    for i in range(L):
        p = f"visual.blocks.{i}."
        s.update({p + "norm1.weight": (D,), p + "norm1.bias": (D,),
                  p + "attn.q_bias": (D,), p + "attn.v_bias": (D,),
                  p + "attn.qkv.weight": (3 * D, D),
                  p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,),
                  p + "norm2.weight": (D,), p + "norm2.bias": (D,),
                  p + "mlp.fc1.weight": (Dm, D), p + "mlp.fc1.bias": (Dm,),
                  p + "mlp.fc2.weight": (D, Dm), p + "mlp.fc2.bias": (D,)})
    s.update({"visual.norm.weight": (D,), "visual.norm.bias": (D,),
              "visual.head.weight": (E, D), "visual.head.bias": (E,)})
    return s


def eva_text_shapes(cfg: dict) -> Dict[str, Tuple[int, ...]]:
    t = cfg["text_cfg"]
    D, L, E = t["width"], t["layers"], cfg["embed_dim"]
    s = {"text.token_embedding.weight": (t["vocab_size"], D),
         "text.positional_embedding": (t["context_length"], D)}
    for i in range(L):
        p = f"text.transformer.resblocks.{i}."
        s.update({p + "ln_1.weight": (D,), p + "ln_1.bias": (D,),
                  p + "attn.in_proj_weight": (3 * D, D), p + "attn.in_proj_bias": (3 * D,),
                  p + "attn.out_proj.weight": (D, D), p + "attn.out_proj.bias": (D,),
                  p + "ln_2.weight": (D,), p + "ln_2.bias": (D,),
                  p + "mlp.c_fc.weight": (4 * D, D), p + "mlp.c_fc.bias": (4 * D,),
                  p + "mlp.c_proj.weight": (D, 4 * D), p + "mlp.c_proj.bias": (D,)})
    s.update({"text.ln_final.weight": (D,), "text.ln_final.bias": (D,),
              "text.text_projection": (D, E), "text.logit_scale": ()})
    return s


def _layer_index(name: str) -> int:
    parts = name.split(".")
    for a, b in zip(parts, parts[1:]):
        if a in ("blocks", "resblocks", "layer") and b.isdigit():
            return int(b)
    return 0


def _init_rule(name: str, shape) -> Tuple[float, float]:
    """(std, mean) per tensor.  Scales follow the reference's own initialisers
    (vit_model.py:291-318 trunc_normal .02 with proj/fc2 / sqrt(2*layer);
    eva_model.py:206-222) but biases and LayerNorm affines are made non-trivial so
    that every bias / affine code path is exercised by the parity tests."""
    leaf = name.split(".")[-1]
    if name.endswith("logit_scale"):
        return 0.0, math.log(1 / 0.07)
    if "norm" in name or ".ln_" in name or "ln_final" in name or "ln_pre" in name or "ln_post" in name \
            or "LayerNorm" in name:
        return (0.1, 1.0) if leaf == "weight" else (0.05, 0.0)
    if leaf in ("bias", "q_bias", "v_bias", "in_proj_bias"):
        return 0.02, 0.0
    if name.endswith("token_embedding.weight"):
        return 0.02, 0.0
    if name.endswith("positional_embedding") or name.endswith("pos_embed") or name.endswith("cls_token") \
            or name.endswith("class_embedding"):
        return 0.02, 0.0
    if name.endswith("qkv.weight") or name.endswith("in_proj_weight"):
        return 0.04, 0.0
    if name.endswith("attn.proj.weight") or name.endswith("fc2.weight") \
            or name.endswith("out_proj.weight") or name.endswith("c_proj.weight"):
        return 0.02 / math.sqrt(2.0 * (_layer_index(name) + 1)), 0.0
    if name.endswith("text_projection") or name.endswith("visual.proj"):
        return shape[0] ** -0.5, 0.0
    return 0.02, 0.0


def state_dict(shapes: Dict[str, Tuple[int, ...]], seed: int) -> Dict[str, torch.Tensor]:
    # tensors are independent pure functions of (name, seed): generate them on a few threads (numpy releases the GIL)
    import os
    from concurrent.futures import ThreadPoolExecutor

    def make(item):
        name, shape = item
        std, mean = _init_rule(name, shape)
        return name, tensor(name, shape, std, seed, mean)
    items = list(shapes.items())
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as ex:
        out = dict(ex.map(make, items))
    # the decoder's input embedding and its LM-head matrix are ONE tied parameter in the reference
    # (module_decoder.py:171-176,284-285): a checkpoint carries the same values under both names
    tied_a = "clip4cap_model.decoder.embeddings.word_embeddings.weight"
    tied_b = "clip4cap_model.decoder.classifier.cls.predictions.decoder.weight"
    if tied_a in out and tied_b in out:
        out[tied_a] = out[tied_b]
    return out


def eva_clip_state_dict(cfg: dict, seed: int, towers=("visual", "text")) -> Dict[str, torch.Tensor]:
    shapes = {}
    if "visual" in towers:
        shapes.update(eva_vision_shapes(cfg))
    if "text" in towers:
        shapes.update(eva_text_shapes(cfg))
    return state_dict(shapes, seed)


# ----------------------------------------------------------------------------------
# OpenAI CLIP ViT-B/32 as vendored in the reference (EVA_clip/model.py)
# ----------------------------------------------------------------------------------

OPENAI_VIT_B32 = {"embed_dim": 512, "image_resolution": 224, "vision_layers": 12, "vision_width": 768,
                  "vision_patch_size": 32, "context_length": 77, "vocab_size": 49408,
                  "transformer_width": 512, "transformer_heads": 8, "transformer_layers": 12}

OPENAI_VIT_TINY = {"embed_dim": 64, "image_resolution": 224, "vision_layers": 2, "vision_width": 128,
                   "vision_patch_size": 32, "context_length": 77, "vocab_size": 49408,
                   "transformer_width": 128, "transformer_heads": 2, "transformer_layers": 2}


def openai_clip_shapes(c: dict) -> Dict[str, Tuple[int, ...]]:
    W, P, E = c["vision_width"], c["vision_patch_size"], c["embed_dim"]
    G = c["image_resolution"] // P
    s = {"visual.conv1.weight": (W, 3, P, P), "visual.class_embedding": (W,),
         "visual.positional_embedding": (G * G + 1, W),
         "visual.ln_pre.weight": (W,), "visual.ln_pre.bias": (W,)}

    def blocks(prefix, D, L):
        for i in range(L):
            p = f"{prefix}.resblocks.{i}."
            s.update({p + "attn.in_proj_weight": (3 * D, D), p + "attn.in_proj_bias": (3 * D,),
                      p + "attn.out_proj.weight": (D, D), p + "attn.out_proj.bias": (D,),
                      p + "ln_1.weight": (D,), p + "ln_1.bias": (D,),
                      p + "mlp.c_fc.weight": (4 * D, D), p + "mlp.c_fc.bias": (4 * D,),
                      p + "mlp.c_proj.weight": (D, 4 * D), p + "mlp.c_proj.bias": (D,),
                      p + "ln_2.weight": (D,), p + "ln_2.bias": (D,)})

    blocks("visual.transformer", W, c["vision_layers"])
    s.update({"visual.ln_post.weight": (W,), "visual.ln_post.bias": (W,), "visual.proj": (W, E)})
    T = c["transformer_width"]
    blocks("transformer", T, c["transformer_layers"])
    s.update({"token_embedding.weight": (c["vocab_size"], T),
              "positional_embedding": (c["context_length"], T),
              "ln_final.weight": (T,), "ln_final.bias": (T,),
              "text_projection": (T, E), "logit_scale": ()})
    return s


def openai_clip_state_dict(c: dict, seed: int) -> Dict[str, torch.Tensor]:
    return state_dict(openai_clip_shapes(c), seed)


# ----------------------------------------------------------------------------------
# Joint model (MomentModel minus the frozen EVA-CLIP): schema = the reference's own state-dict keys
# (tests/golden/joint_schema.json, dumped from the real module)
# ----------------------------------------------------------------------------------

def joint_state_dict(shapes: Dict[str, Tuple[int, ...]], seed: int) -> Dict[str, torch.Tensor]:
    out = {}
    for name, shape in shapes.items():
        leaf = name.split(".")[-1]
        if "LayerNorm" in name or "visual_norm2d" in name or name.startswith("asr_enc_layer.0"):
            std, mean = (0.1, 1.0) if leaf == "weight" else (0.05, 0.0)
        elif leaf == "bias":
            std, mean = 0.02, 0.0
        elif "predictor" in name:
            std, mean = 0.05, 0.0
        elif name.endswith("query.weight") or name.endswith("key.weight"):
            std, mean = 0.06, 0.0          # non-trivial attention logits
        elif "embed" in name.lower():
            std, mean = 0.05, 0.0
        else:
            std, mean = 0.03, 0.0
        out[name] = tensor(name, shape, std, seed, mean)
    # the decoder's input embedding and its LM-head matrix are ONE tied parameter in the reference
    # (module_decoder.py:171-176,284-285): a checkpoint carries the same values under both names
    tied_a = "clip4cap_model.decoder.embeddings.word_embeddings.weight"
    tied_b = "clip4cap_model.decoder.classifier.cls.predictions.decoder.weight"
    if tied_a in out and tied_b in out:
        out[tied_a] = out[tied_b]
    return out


# ----------------------------------------------------------------------------------
# ASR sentence encoder: sentence-transformers/all-MiniLM-L6-v2 = a 6-layer BERT (extraction/whisper_ASR/extract_ASR_embedding.py:14)
# in the Hugging Face BertModel checkpoint schema (the file sentence-transformers loads with AutoModel)
# ----------------------------------------------------------------------------------

MINILM_L6 = {"vocab_size": 30522, "hidden_size": 384, "num_hidden_layers": 6, "num_attention_heads": 12,
             "intermediate_size": 1536, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12}
MINILM_TINY = {"vocab_size": 700, "hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 2,
               "intermediate_size": 128, "max_position_embeddings": 64, "type_vocab_size": 2, "layer_norm_eps": 1e-12}


def bert_shapes(c: dict) -> Dict[str, Tuple[int, ...]]:
    D, I = c["hidden_size"], c["intermediate_size"]
    s = {"embeddings.word_embeddings.weight": (c["vocab_size"], D),
         "embeddings.position_embeddings.weight": (c["max_position_embeddings"], D),
         "embeddings.token_type_embeddings.weight": (c["type_vocab_size"], D),
         "embeddings.LayerNorm.weight": (D,), "embeddings.LayerNorm.bias": (D,)}
    for i in range(c["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for n in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            s[p + n + ".weight"] = (D, D)
            s[p + n + ".bias"] = (D,)
        s.update({p + "attention.output.LayerNorm.weight": (D,), p + "attention.output.LayerNorm.bias": (D,),
                  p + "intermediate.dense.weight": (I, D), p + "intermediate.dense.bias": (I,),
                  p + "output.dense.weight": (D, I), p + "output.dense.bias": (D,),
                  p + "output.LayerNorm.weight": (D,), p + "output.LayerNorm.bias": (D,)})
    s.update({"pooler.dense.weight": (D, D), "pooler.dense.bias": (D,)})   # in the checkpoint, unused by mean pooling
    return s


def bert_state_dict(c: dict, seed: int) -> Dict[str, torch.Tensor]:
    return joint_state_dict(bert_shapes(c), seed)


# BERTScore's encoder (bert_score.score(lang='en') = roberta-large cut after layer 17, evaluate.py:294-297) in the Hugging Face
# RobertaModel checkpoint schema: BERT's layers, one token-type row, positions offset by pad_token_id + 1.  ROBERTA_WIDE has
# roberta-large's widths with few layers; ROBERTA_LARGE only shapes tools/bertscore_bench.py.
ROBERTA_TINY = {"model_type": "roberta", "vocab_size": 700, "hidden_size": 64, "num_hidden_layers": 4, "num_attention_heads": 4,
                "intermediate_size": 128, "max_position_embeddings": 68, "type_vocab_size": 1, "layer_norm_eps": 1e-5,
                "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2}
ROBERTA_WIDE = {"model_type": "roberta", "vocab_size": 1000, "hidden_size": 1024, "num_hidden_layers": 3, "num_attention_heads": 16,
                "intermediate_size": 4096, "max_position_embeddings": 514, "type_vocab_size": 1, "layer_norm_eps": 1e-5,
                "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2}
ROBERTA_LARGE = dict(ROBERTA_WIDE, num_hidden_layers=24)


def roberta_state_dict(c: dict, seed: int, num_layers: int = None) -> Dict[str, torch.Tensor]:
    """Seeded weights under a roberta checkpoint's names (``roberta.`` prefix, no pooler); ``num_layers``: only the first so many
    layers (the values of a tensor depend on its name and the seed alone, so a cut dict equals the full one's first layers)."""
    if num_layers is not None:
        c = dict(c, num_hidden_layers=num_layers)
    return {"roberta." + k: v for k, v in joint_state_dict({k: s for k, s in bert_shapes(c).items() if not k.startswith("pooler.")},
                                                           seed).items()}


def sentence_ids(name: str, n: int, seed: int, vocab_size: int, min_len: int = 2, max_len: int = 40,
                 cls_id: int = 101, sep_id: int = 102) -> list:
    """n ragged rows [CLS] w.. [SEP] with lengths spread over [min_len, max_len] (min_len 2 = an empty subtitle)"""
    u = (uniform_pm1(name + ".len", n, seed) + 1.0) * 0.5
    rows = []
    for r in range(n):
        L = min_len + int(u[r] * (max_len - min_len + 1))
        L = min(max(L, 2), max_len)
        body = ((uniform_pm1(f"{name}.row{r}", L - 2, seed) + 1.0) * 0.5 * (vocab_size - 200)).astype(np.int64) + 200 if L > 2 \
            else np.zeros(0, np.int64)
        rows.append([cls_id] + [int(x) for x in body] + [sep_id])
    return rows


# ----------------------------------------------------------------------------------
# Seeded input builders of the joint-model / evaluation / timeline fixtures.  tests/golden/make_golden.py feeds these to the
# real reference; the GPU tests, tools/ and bench.py rebuild the same inputs from here (nothing in them touches the reference).
# ----------------------------------------------------------------------------------

def joint_inputs(name, B, T, seed):
    """C4-style synthetic batch: L2-normalised frame features, sparse ASR features, ragged lengths."""
    vis = tensor(f"{name}.vis", (B, T, 1024), 1.0, seed)
    vis = vis / vis.norm(dim=-1, keepdim=True)
    asr = tensor(f"{name}.asr", (B, T, 384), 0.05, seed)
    gaps = uniform_pm1(f"{name}.gap", B * T, seed).reshape(B, T) > 0.2      # ~40 % all-zero rows
    asr = asr * torch.from_numpy(~gaps).float()[..., None]
    text = tensor(f"{name}.text", (B, 1024), 1.0, seed)
    lens = [T - (b * T) // (3 * B) for b in range(B)]                             # ragged
    vis_mask = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        vis_mask[b, :n] = 1
        vis[b, n:] = 0
        asr[b, n:] = 0
    bounds = torch.tensor([[int(0.1 * n), int(0.8 * n)] for n in lens], dtype=torch.long)
    moment_mask = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        moment_mask[b, bounds[b, 0]:bounds[b, 1] + 1] = 1
    return vis, asr, text, vis_mask, moment_mask, bounds


TRAIN_CASES = {"a": (3, 64), "b": (2, 300)}
# step-captioning goldens (tests/golden/caption_predictions.json): case -> (B, T, beams, moment lengths)
CAPTION_CASES = {"a": (3, 64, 3, [7, 20, 37]), "b": (2, 300, 5, [7, 20]),
                 "c3": (5, 300, 3, [15] * 5), "c5": (5, 300, 5, [15] * 5),
                 # the reference's default evaluation batch (args.py:27 --eval_batch_size 32): 96 / 160 beam rows per word, moments
                 # shorter than, equal to and longer than max_frames mixed in one batch
                 "d3": (32, 300, 3, [[15, 7, 20, 37, 12, 25, 3, 18][b % 8] for b in range(32)]),
                 "d5": (32, 300, 5, [[15, 7, 20, 37, 12, 25, 3, 18][b % 8] for b in range(32)])}


def train_targets(name, B, T, seed, bounds):
    """start / end targets inside the moment, a previous-boundary mask and a segmentation target (hirest_dataset.py:409-531 keys)."""
    u = (uniform_pm1(f"{name}.tgt", 4 * B, seed).reshape(4, B) + 1.0) * 0.5
    lo, hi = bounds[:, 0].numpy(), bounds[:, 1].numpy()
    st = (lo + u[0] * (hi - lo)).astype(np.int64)
    et = np.maximum(st, (lo + u[1] * (hi - lo)).astype(np.int64))
    seg = (lo + u[2] * (hi - lo)).astype(np.int64)
    prev = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        prev[b, int(lo[b])] = 1
    return torch.from_numpy(st), torch.from_numpy(et), torch.from_numpy(seg), prev


def caption_targets(name, B, max_words, seed):
    """Teacher-forcing triples in the reference's target_text 9-tuple layout (fields 5, 6, 7: decoder input ids, decoder mask,
    output ids with -1 on the padding): [CLS] w1 .. wn  /  w1 .. wn [SEP]."""
    u = (uniform_pm1(f"{name}.cap", B * (max_words + 1), seed).reshape(B, max_words + 1) + 1.0) * 0.5
    out = []
    for b in range(B):
        n = 3 + int(u[b, 0] * (max_words - 8))
        words = (1000 + (u[b, 1:1 + n] * 29000)).astype(np.int64).tolist()
        inp = [101] + words + [0] * (max_words - 1 - n)
        mask = [1] * (n + 1) + [0] * (max_words - 1 - n)
        outp = words + [102] + [-1] * (max_words - 1 - n)
        out.append((None, None, None, None, None, inp, mask, outp, None))
    return out


def valid_batches(case, max_words=48):
    """The three loader-shaped batches of one TRAIN_CASES case for the validation pass (tests/golden/valid_*.json): the inputs and
    targets of the training fixtures plus the per-sample lists run.py's predict() collects (``tasks``, ``prompts``, ``video_fnames``,
    ``video_duration``).  Durations sit just above each video's valid frames (one bin per second), except one segmentation sample
    whose duration is shorter than its moment — its timestamps raise, which is the short-``bounds`` case of run.py:766-774 — and two
    captioning samples share a video name."""
    B, T = TRAIN_CASES[case]
    vis, asr, text, vis_mask, moment_mask, bounds = joint_inputs(f"train.{case}", B, T, 53)
    st, et, seg, prev = train_targets(f"train.{case}", B, T, 53, bounds)
    lens = vis_mask.sum(1).tolist()
    videos = [f"video_{case}{b}" for b in range(B)]
    common = {"vis_feats": vis, "vis_mask": vis_mask, "asr_feats": asr, "text_feat": text, "prompts": [f"prompt {case}{b % 2}" for b in range(B)],
              "video_fnames": videos, "video_duration": [n + 0.25 for n in lens]}
    retrieval = dict(common, tasks=["moment_retrieval"] * B, moment_mask=moment_mask, moment_retrieval_start_target=st,
                     moment_retrieval_end_target=et)
    short = list(common["video_duration"])
    short[B - 1] = float(int(bounds[B - 1, 0]) + 3)
    segmentation = dict(common, tasks=["moment_segmentation"] * B, moment_mask=moment_mask, prev_boundary_mask=prev,
                        moment_segmentation_target=seg, moment_bound_frames=bounds, video_duration=short,
                        all_bound_frames=[[int(bounds[b, 0]), int(seg[b]), int(bounds[b, 1])] for b in range(B)])
    cap_mask = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate([7, 20, 37][:B]):
        cap_mask[b, 5 + b:5 + b + n] = 1
    captioning = dict(common, tasks=["step_captioning"] * B, moment_mask=cap_mask, target_text=caption_targets(f"train.{case}", B, max_words, 53),
                      target_text_raw=[f"step {case}{b}" for b in range(B)], video_fnames=[videos[0]] + videos[:B - 1])
    return {"moment_retrieval": retrieval, "moment_segmentation": segmentation, "step_captioning": captioning}


def moment_eval_inputs():
    """Seeded synthetic gt / predictions in evaluate.py's JSON layouts (shared with tests/test_evaluation.py)."""
    cats = ["Food", "Hobbies", "Home"]
    u = uniform_pm1("moment_eval", 20000, 17)
    it = iter(((u + 1.0) * 0.5).tolist())
    rnd = lambda lo, hi: lo + (hi - lo) * next(it)
    prompt_to_cat, video_to_cat = {}, {}
    mr_gt, mr_pred, sb_gt, sb_pred = {}, {}, {}, {}
    for pi in range(24):
        prompt = f"prompt {pi}"
        prompt_to_cat[prompt] = cats[pi % 3]
        mr_gt[prompt], mr_pred[prompt] = {}, {}
        for vi in range(1 + pi % 3):
            video = f"vid_{pi}_{vi}.mp4"
            video_to_cat[video] = cats[(pi + vi) % 3]
            dur = int(rnd(40, 600))
            a = int(rnd(0, dur * 0.6)); b = a + 1 + int(rnd(2, dur * 0.4))
            clip = (pi + vi) % 5 != 0
            mr_gt[prompt][video] = {"clip": clip, "bounds": [a, b], "v_duration": dur}
            mode = (pi + 2 * vi) % 6
            if mode == 0:
                pb = [a, b]                                            # exact
            elif mode == 1:
                pb = [b + 3, b + 9]                                    # disjoint
            elif mode == 2:
                pb = [a, a + (b - a) // 2]                             # IoU near 0.5
            else:
                pb = [max(0, a + int(rnd(-15, 15))), b + int(rnd(-15, 15))]
                if pb[1] <= pb[0]:
                    pb[1] = pb[0] + 1
            mr_pred[prompt][video] = {"bounds": pb}
            if clip:
                n_steps = 2 + int(rnd(0, 7))
                cuts = sorted(set([a, b] + [int(rnd(a + 1, b - 1)) for _ in range(n_steps)]))
                refs = [[cuts[i], cuts[i + 1]] for i in range(len(cuts) - 1)]
                sb_gt[video] = {"bounds": refs}
                preds = []
                for r in refs:                                         # jittered, duplicated, nested and outside boxes
                    if next(it) < 0.8:
                        preds.append([r[0] + int(rnd(-3, 4)), r[1] + int(rnd(-3, 4))])
                    if next(it) < 0.3:
                        preds.append([r[0] + 1, r[1] - 1] if r[1] - r[0] > 3 else [r[0], r[1]])
                if next(it) < 0.5:
                    preds.append([a - 5, a + 2])
                if next(it) < 0.3:
                    preds.append([rnd(a, b), rnd(a, b) + 2.5])         # float bounds
                preds = [p if p[1] > p[0] else [p[0], p[0] + 1] for p in preds]
                sb_pred[video] = {"bounds": preds}
    return {"prompt_to_cat": prompt_to_cat, "video_to_cat": video_to_cat, "mr_gt": mr_gt, "mr_pred": mr_pred,
            "sb_gt": sb_gt, "sb_pred": sb_pred}


def timeline_cases():
    """Inputs of the frame-index <-> timestamp fixture (pure numpy; shared with tests/test_timeline.py): per case the
    frame indices 0..n-1 and a timestamp list holding a regular sweep past the end, every bin value exactly, and the
    doubles just below / above every bin (the digitize(right=True) edge)."""
    cases = []
    for dur in (1.0, 1.9, 2.0, 3.7, 17.3, 59.9, 60.0, 199.99, 200.0, 367.8, 571.4, 1855.2, 2500.5):
        for n in (-1, 1, 2, 3, 20, 32, 64, 300, 2048):
            nn = int(dur) if n < 0 else n
            bins = np.linspace(0, int(dur) - 1, nn)
            t = np.concatenate([np.arange(-1.0, dur + 3.0, 0.37), bins, np.nextafter(bins, -np.inf), np.nextafter(bins, np.inf),
                                np.arange(0, int(dur) + 2, dtype=np.float64)])
            cases.append({"duration": dur, "n_frames": n, "frames": np.arange(nn, dtype=np.int64), "timestamps": t})
    return cases




# ----------------------------------------------------------------------------------
# BASELINE configs[2] sub-corpus of the matched-R@k check: tests/golden/make_golden.py encodes it with the real
# reference; bench.py and the GPU tests re-encode it with the kernels.
# ----------------------------------------------------------------------------------

def c3_corpus(V: int, F: int) -> torch.Tensor:
    """video v's frames = base_v + 0.1 * noise_{v,f} (non-degenerate, seeded): [V, F, 3, 224, 224] fp32."""
    base = frames("c3.base", (V, 1, 3, 224, 224), 5)
    return base + 0.1 * frames("c3.noise", (V, F, 3, 224, 224), 6)


def c3_names(V: int) -> list:
    """File names deliberately NOT in index order under string sort, so the (score, name) tie rule of evaluate.py:58-60 is
    exercised; unique for V <= 257."""
    assert V <= 257
    return [f"vid_{(v * 37) % 257:03d}.mp4" for v in range(V)]


# ----------------------------------------------------------------------------------
# BASELINE configs[2] through the feature-file branch (inference_video_retrieval.py:290-355): one [T_v, E] "feature file" per
# video of a corpus, T_v between 3 and 42 rows (below and above any n_model_frames the tests use, so the linspace
# subsample both repeats and drops rows).  tests/golden/make_golden.py gen_retrieval_run writes these files and runs the
# REAL script over them; the tests regenerate the same tensors.
# ----------------------------------------------------------------------------------

def retrieval_feature_lengths(n_videos: int, seed: int = 9) -> np.ndarray:
    u = uniform_pm1("vr.len", n_videos, seed)
    return (3 + np.floor((u + 1.0) * 20.0)).astype(np.int64).clip(3, 42)


def retrieval_feature_corpus(n_videos: int, embed_dim: int, seed: int = 9) -> list:
    """[n_videos] fp32 tensors [T_v, embed_dim]; rows ~ unit-variance noise around a per-video offset (so pooled rows differ)."""
    lens = retrieval_feature_lengths(n_videos, seed)
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = tensor("vr.rows", (int(off[-1]), embed_dim), 1.0, seed)
    base = tensor("vr.base", (n_videos, embed_dim), 1.0, seed + 1)
    return [rows[off[v]:off[v + 1]] * 0.25 + base[v] for v in range(n_videos)]


def c3_device_block(lo: int, hi: int, n_frames: int, device, dtype=torch.bfloat16) -> torch.Tensor:
    """Videos [lo, hi) of the full-size C3 corpus (base_v + 0.1 * noise_f), generated ON the device from a
    per-video seed — 4096 x 32 frames would be 79 GB of host fp32 — so any partition of the corpus (one sweep, 8 rank
    blocks, 8 real ranks) regenerates identical inputs.  torch's Philox stream: stable for a given torch build, which is
    why the committed digests are keyed by torch.__version__."""
    out = torch.empty((hi - lo, n_frames, 3, 224, 224), device=device, dtype=dtype)
    for i, v in enumerate(range(lo, hi)):
        gen = torch.Generator(device=device)
        gen.manual_seed(100000 + v)
        base = torch.randn((1, 3, 224, 224), device=device, generator=gen)
        out[i] = (base + 0.1 * torch.randn((n_frames, 3, 224, 224), device=device, generator=gen)).to(dtype)
    return out


def c3_device_names(V: int) -> list:
    """Unique file names whose string order is not the corpus order (the tie rule of evaluate.py:58-60 sorts by name)."""
    assert V <= 10007
    return [f"video_{(v * 7919) % 10007:05d}.mp4" for v in range(V)]


# ----------------------------------------------------------------------------------
# Whisper's audio encoder (extraction/whisper_ASR/extract_ASR.py:  whisper.load_model('small.en')) in the Hugging Face WhisperEncoder
# checkpoint schema, config keys as in its config.json.  WHISPER_SMALL_EN only shapes tools/whisper_bench.py; the lettered configs are the
# cases of tests/golden/whisper_enc_*.npz (a: odd ctx, ragged in every tile, 64-wide heads; b: 32-wide heads; c: Whisper-tiny's width,
# whose second convolution takes the fp32 GEMM's split form, M > 256 and K >= 1024); WHISPER_E2E has the real 1500-token context.
# ----------------------------------------------------------------------------------

WHISPER_SMALL_EN = {"num_mel_bins": 80, "d_model": 768, "encoder_attention_heads": 12, "encoder_layers": 12, "encoder_ffn_dim": 3072,
                    "max_source_positions": 1500}
WHISPER_TINY_A = {"num_mel_bins": 80, "d_model": 128, "encoder_attention_heads": 2, "encoder_layers": 2, "encoder_ffn_dim": 512,
                  "max_source_positions": 33}
WHISPER_TINY_B = {"num_mel_bins": 80, "d_model": 128, "encoder_attention_heads": 4, "encoder_layers": 2, "encoder_ffn_dim": 512,
                  "max_source_positions": 97}
WHISPER_TINY_C = {"num_mel_bins": 80, "d_model": 384, "encoder_attention_heads": 6, "encoder_layers": 1, "encoder_ffn_dim": 1536,
                  "max_source_positions": 261}
WHISPER_E2E = {"num_mel_bins": 80, "d_model": 128, "encoder_attention_heads": 2, "encoder_layers": 1, "encoder_ffn_dim": 512,
               "max_source_positions": 1500}
WHISPER_CASES = {"a": (WHISPER_TINY_A, 3), "b": (WHISPER_TINY_B, 2), "c": (WHISPER_TINY_C, 1)}      # case -> (config, clips)


def whisper_encoder_shapes(c: dict) -> Dict[str, Tuple[int, ...]]:
    D, F, M = c["d_model"], c["encoder_ffn_dim"], c["num_mel_bins"]
    s = {"conv1.weight": (D, M, 3), "conv1.bias": (D,), "conv2.weight": (D, D, 3), "conv2.bias": (D,),
         "embed_positions.weight": (c["max_source_positions"], D)}
    for i in range(c["encoder_layers"]):
        p = f"layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"] = (D, D)
            if n != "k_proj":                                   # Whisper's key projection has no bias
                s[p + f"self_attn.{n}.bias"] = (D,)
        s.update({p + "self_attn_layer_norm.weight": (D,), p + "self_attn_layer_norm.bias": (D,),
                  p + "fc1.weight": (F, D), p + "fc1.bias": (F,), p + "fc2.weight": (D, F), p + "fc2.bias": (D,),
                  p + "final_layer_norm.weight": (D,), p + "final_layer_norm.bias": (D,)})
    s.update({"layer_norm.weight": (D,), "layer_norm.bias": (D,)})
    return s


def whisper_encoder_state_dict(c: dict, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded encoder weights under WhisperEncoder's names: LayerNorm weights spread around 1, query / key weights wide enough for a
    non-uniform attention, every bias non-zero."""
    out = {}
    for name, shape in whisper_encoder_shapes(c).items():
        leaf = name.split(".")[-1]
        if "layer_norm" in name:
            std, mean = (0.1, 1.0) if leaf == "weight" else (0.05, 0.0)
        elif leaf == "bias":
            std, mean = 0.02, 0.0
        elif "q_proj" in name or "k_proj" in name:
            std, mean = 0.06, 0.0
        elif name.startswith("embed_positions") or name.startswith("conv1"):
            std, mean = 0.05, 0.0
        else:
            std, mean = 0.03, 0.0
        out[name] = tensor("whisper." + name, shape, std, seed, mean)
    return out


def whisper_mel_input(c: dict, clips: int, seed: int) -> torch.Tensor:
    """A mel-like encoder input [clips, num_mel_bins, 2 * max_source_positions], uniform in [-0.7, 1.3) (a log-mel spectrogram's range)."""
    shape = (clips, c["num_mel_bins"], 2 * c["max_source_positions"])
    return torch.from_numpy((uniform_pm1("whisper.mel", int(np.prod(shape)), seed) + 0.3).astype(np.float32).reshape(shape))


# the log-mel cases of tests/golden/whisper_mel.npz: case -> (kind, samples, padding)
AUDIO_CASES = {"silence": ("silence", 1600, 0), "tone_noise": ("tone_noise", 1000, 0), "noise": ("noise", 16000, 0),
               "click": ("click", 8000, 0), "mixed": ("mixed", 330000, 150000)}


def audio_clip(kind: str, n: int, seed: int) -> np.ndarray:
    """n seeded float32 samples of 16 kHz mono audio.  The sine of the tone is rounded to the PCM16 grid, so a last-bit difference between
    two libm builds cannot reach the samples; everything else is exact arithmetic on uniform_pm1."""
    t = np.arange(n, dtype=np.float64)
    noise = uniform_pm1(f"audio.{kind}", n, seed)
    tone = np.round(0.5 * np.sin(2.0 * np.pi * 440.0 * t / 16000.0) * 32768.0) / 32768.0
    if kind == "silence":
        x = np.zeros(n)
    elif kind == "tone_noise":
        x = tone + 0.1 * noise
    elif kind == "noise":
        x = 0.3 * noise
    elif kind == "click":                      # one full-scale sample in noise so low that most of the spectrogram sits on the max - 8 clamp
        x = 5e-6 * noise
        x[n // 2] = 1.0
    elif kind == "mixed":                      # 7 s of tone, then noise, then near-silence
        a, b = min(n, 7 * 16000), min(n, 14 * 16000)
        x = np.concatenate([tone[:a] + 0.01 * noise[:a], 0.2 * noise[a:b], 1e-4 * noise[b:]])
    else:
        raise ValueError(f"unknown audio kind {kind!r}")
    return x.astype(np.float32)


# ----------------------------------------------------------------------------------
# Whisper's text decoder in the Hugging Face WhisperDecoder schema (tests/golden/whisper_dec_*.npz).  The vocabularies follow small.en's
# layout: text ids, then eot, sot, the task and marker tokens, <|notimestamps|>, and the timestamp tokens up to the end.
# p: one ragged key chunk; q: several chunks with a ragged last one; r: the real key count and vocabulary width, one layer.
# ----------------------------------------------------------------------------------

def _dec_config(d, heads, layers, audio_ctx, vocab, text_ctx):
    return {"num_mel_bins": 80, "d_model": d, "encoder_attention_heads": heads, "encoder_layers": 1, "encoder_ffn_dim": 4 * d,
            "max_source_positions": audio_ctx, "decoder_attention_heads": heads, "decoder_layers": layers, "decoder_ffn_dim": 4 * d,
            "vocab_size": vocab, "max_target_positions": text_ctx}


def whisper_special_tokens(eot: int) -> Dict[str, int]:
    """small.en's special-token layout shifted to a vocabulary whose text ids end at ``eot`` (50256 there): 99 language slots are kept only at
    the real size, so timestamp_begin = eot + 107 at 50256 and eot + 12 otherwise."""
    base = eot + 1 + (99 if eot == 50256 else 4)
    return {"<|endoftext|>": eot, "<|startoftranscript|>": eot + 1, "<|translate|>": base + 1, "<|transcribe|>": base + 2,
            "<|startoflm|>": base + 3, "<|startofprev|>": base + 4, "<|nospeech|>": base + 5, "<|notimestamps|>": base + 6}


WHISPER_DEC_P = _dec_config(128, 2, 2, 33, 200, 48)
WHISPER_DEC_Q = _dec_config(128, 2, 2, 261, 200, 48)
WHISPER_DEC_R = _dec_config(256, 4, 1, 1500, 51864, 32)
# case -> (config, eot, decoder seed, windows)
WHISPER_DEC_CASES = {"p": (WHISPER_DEC_P, 100, 81, 1), "q": (WHISPER_DEC_Q, 100, 82, 2), "r": (WHISPER_DEC_R, 50256, 83, 1)}
# The widths and head counts of the released checkpoints (tests/test_gpu_whisper_widths.py), one layer and 70 audio positions each (two key
# chunks, the second ragged).  s: small.en's width with a vocabulary past 8192 columns, where the LM head takes the branches 51864 takes;
# w384 / w512 / w1024 / w1280: tiny's, base's, medium's and large's width.
WHISPER_DEC_S = _dec_config(768, 12, 1, 70, 8200, 24)
WHISPER_DEC_CASES.update({"s": (WHISPER_DEC_S, 8000, 84, 3),
                          "w384": (_dec_config(384, 6, 1, 70, 200, 16), 100, 85, 1), "w512": (_dec_config(512, 8, 1, 70, 200, 16), 100, 86, 1),
                          "w1024": (_dec_config(1024, 16, 1, 70, 200, 16), 100, 87, 1),
                          "w1280": (_dec_config(1280, 20, 1, 70, 200, 16), 100, 88, 1)})
WHISPER_DEC_WIDTH_CASES = ("s", "w384", "w512", "w1024", "w1280")
# A text context of 160, so that prompts of more than one and more than two 64-query attention blocks exist (65 and 130 tokens:
# tests/test_gpu_whisper_prefill.py).  (config, eot, decoder seed, windows) as an entry of WHISPER_DEC_CASES, kept out of that table:
# it has no fixture — the yardstick of a ragged prefill is the per-window prefill of the same weights.
WHISPER_DEC_LONG = (_dec_config(128, 2, 1, 70, 200, 160), 100, 89, 3)


def whisper_decoder_shapes(c: dict) -> Dict[str, Tuple[int, ...]]:
    D, F = c["d_model"], c["decoder_ffn_dim"]
    s = {"embed_tokens.weight": (c["vocab_size"], D), "embed_positions.weight": (c["max_target_positions"], D)}
    for i in range(c["decoder_layers"]):
        p = f"layers.{i}."
        for a in ("self_attn", "encoder_attn"):
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                s[p + f"{a}.{n}.weight"] = (D, D)
                if n != "k_proj":
                    s[p + f"{a}.{n}.bias"] = (D,)
            s[p + f"{a}_layer_norm.weight"] = s[p + f"{a}_layer_norm.bias"] = (D,)
        s.update({p + "fc1.weight": (F, D), p + "fc1.bias": (F,), p + "fc2.weight": (D, F), p + "fc2.bias": (D,),
                  p + "final_layer_norm.weight": (D,), p + "final_layer_norm.bias": (D,)})
    s.update({"layer_norm.weight": (D,), "layer_norm.bias": (D,)})
    return s


def whisper_decoder_state_dict(c: dict, seed: int, eot: Optional[int] = None, eot_bias: float = 0.0) -> Dict[str, torch.Tensor]:
    """Seeded decoder weights under ``decoder.`` + WhisperDecoder's names.  The embedding (also the LM head) is wide enough for logits
    that differ by whole units.  ``eot_bias`` adds that multiple of the final LayerNorm's bias direction to the eot embedding, which moves
    the eot logit of every position by about the same amount: how a fixture is made to end by eot."""
    out = {}
    for name, shape in whisper_decoder_shapes(c).items():
        leaf = name.split(".")[-1]
        if "layer_norm" in name:
            std, mean = (0.1, 1.0) if leaf == "weight" else (0.05, 0.0)
        elif leaf == "bias":
            std, mean = 0.02, 0.0
        elif "q_proj" in name or "k_proj" in name:
            std, mean = 0.06, 0.0
        elif name.startswith("embed_tokens"):
            std, mean = 0.08, 0.0
        elif name.startswith("embed_positions"):
            std, mean = 0.05, 0.0
        else:
            std, mean = 0.03, 0.0
        out["decoder." + name] = tensor("whisper.dec." + name, shape, std, seed, mean)
    if eot is not None and eot_bias != 0.0:
        b = out["decoder.layer_norm.bias"]
        out["decoder.embed_tokens.weight"][eot] += eot_bias * b / float((b * b).sum())
    return out


def whisper_audio_states(c: dict, windows: int, seed: int) -> torch.Tensor:
    """Encoder-state-like decoder input [windows, max_source_positions, d_model] (LayerNorm output scale)"""
    return tensor("whisper.dec.xa", (windows, c["max_source_positions"], c["d_model"]), 1.0, seed)


def whisper_vocab(eot: int) -> Tuple[Dict[str, int], list]:
    """A byte-level vocabulary of ``eot`` text ids for the tokenizer tests: the 256 byte symbols first when they fit (else the printable
    ASCII ones), then a few merges, then unmerged two-symbol strings up to ``eot``."""
    from .bytebpe import bytes_to_unicode
    alphabet = list(bytes_to_unicode().values())
    if eot < 300:
        table = bytes_to_unicode()
        alphabet = [table[b] for b in list(range(32, 127))]
    vocab = {s: i for i, s in enumerate(alphabet)}
    sp = bytes_to_unicode()[ord(" ")]
    merges = []
    for a, b in ((sp, "-"), (sp, "'"), ("t", "h"), ("th", "e"), (sp, "the"), (sp, "a"), ("i", "n")):
        if a in vocab and b in vocab and a + b not in vocab and len(vocab) < eot:
            vocab[a + b] = len(vocab)
            merges.append(f"{a} {b}")
    # the text ids left over (a vocabulary of thousands): two-symbol strings no merge produces, so that encode() is unchanged and every id
    # a decoder can pick has a text
    if len(vocab) < eot:
        for a in alphabet:
            for b in alphabet:
                if len(vocab) == eot:
                    return vocab, merges
                if a + b not in vocab:
                    vocab[a + b] = len(vocab)
    return vocab, merges


# added to the eot embedding along the final LayerNorm's bias (whisper_decoder_state_dict): case p's greedy fixtures end by eot, case q's
# run to sample_len, case s's ends by eot inside its 12 sampled positions
WHISPER_DEC_EOT_BIAS = {"p": 0.5, "q": 0.0, "r": 0.0, "s": 3.0, "w384": 0.0, "w512": 0.0, "w1024": 0.0, "w1280": 0.0}


def token_ids(name: str, n: int, vocab: int, seed: int) -> np.ndarray:
    """n seeded ids in [0, vocab)"""
    return np.minimum(((uniform_pm1(name, n, seed) + 1.0) * 0.5 * vocab).astype(np.int64), vocab - 1)


def whisper_tokenizer(eot: int):
    """The synthetic Whisper tokenizer of a decoder case: whisper_vocab + whisper_special_tokens"""
    from .whisper import Tokenizer
    vocab, merges = whisper_vocab(eot)
    return Tokenizer(vocab, merges, whisper_special_tokens(eot))


def whisper_tail_consts(c: dict, eot: int) -> dict:
    """What decode() derives from that tokenizer and the default options: the ids the logit filters use"""
    tok = whisper_tokenizer(eot)
    suppress = sorted(set(tok.non_speech_tokens) | {tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm, tok.no_speech})
    return {"n_vocab": c["vocab_size"], "eot": tok.eot, "no_speech": tok.no_speech, "no_timestamps": tok.no_timestamps,
            "timestamp_begin": tok.timestamp_begin, "max_initial_timestamp_index": int(round(1.0 / (30.0 / c["max_source_positions"]))),
            "blank": tok.encode(" ")[0], "suppress": suppress}
