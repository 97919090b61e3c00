#!/usr/bin/env python3
"""Generate tests/golden/clipscore.{npz,json} (and clipscore_spans.json): the CLIPScore leg of the reference's step-captioning evaluation, run for real.

Runs only in the build container (needs /root/reference and transformers).  It writes a small set of baseline JPEG frame
directories, imports the reference's own ``evaluate.py`` and calls ``evaluate_moment_summarization`` on them, once with
``--print_per_category`` and once without, with these stand-ins:

* ``language_evaluation``, ``allennlp_models`` and ``bert_score``: constant outputs (their models are not on this machine);
* ``clip``: ``load`` returns a recording model that embeds on the CPU in fp32 with ``oracle.ref_cpu.openai_encode_image(...,
  pip_head=True)`` / ``openai_encode_text`` on the ``openai_tiny`` weights (``synth.openai_clip_state_dict(OPENAI_VIT_TINY, 21)``),
  its ``preprocess`` is ``oracle.preprocess_cpu.image_transform`` of the RGB image (torchvision, which pip clip's transform needs,
  is absent), and ``tokenize`` is ``hirest_amd.tokenizer.tokenize`` (pinned against the reference's tokenizer by tokenizer.npz);
* ``torch.Tensor.to("cuda:N")`` stays on the CPU for the duration of the call.

It records which frame files and which candidate went into every CLIP call, every per-caption score, and both result dicts.  It
also stores transformers' ``CLIPModel`` features (an independent implementation of the pip head) of the same tiny weights on a few
seeded frames and token rows.  The fixture holds data only: the JPEG bytes are written once here, so a different Pillow on
another machine cannot change them.

    python tests/golden/make_clipscore_golden.py
"""
import io
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

from hirest_amd import synth  # noqa: E402
from hirest_amd.tokenizer import tokenize  # noqa: E402
from oracle import preprocess_cpu, ref_cpu  # noqa: E402

SEED = 21                      # the openai_tiny weights
GEOM_A = (72, 96)              # (h, w)
GEOM_B = (80, 64)


def frame_pixels(h, w, k, seed, grey=False):
    """A smooth frame with a moving disc and mild noise: distinct content per frame, small at q95."""
    rng = np.random.default_rng(seed * 1000 + k)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = h * (0.3 + 0.4 * ((k * 7) % 11) / 10), w * (0.2 + 0.6 * ((k * 5) % 13) / 12)
    disc = ((y - cy) ** 2 + (x - cx) ** 2 < (min(h, w) / 4) ** 2).astype(np.float64)
    base = np.stack([x / w * 200 + 30 * np.sin(k / 3), y / h * 180 + 40 * disc, (x + y) / (h + w) * 150 + 90 * disc], -1)
    base += (seed * 37 % 60) + rng.normal(0, 6, base.shape)
    a = np.clip(base, 0, 255).astype(np.uint8)
    if grey:
        return a[..., 1]
    return a


def jpeg_bytes(a, progressive=False):
    b = io.BytesIO()
    img = Image.fromarray(a)
    kw = {"quality": 95}
    if img.mode == "RGB":
        kw["subsampling"] = 2                                   # 4:2:0, as cv2.imwrite writes
    if progressive:
        kw["progressive"] = True
    img.save(b, "JPEG", **kw)
    return b.getvalue()


# (video, frames, geometry, name pattern, grey, progressive frame ids)
VIDEOS = [
    ("nWBuM3LNTcM.mp4", 40, GEOM_A, "frame_{:06d}.jpg", False, {17}),
    ("l2OTMq4aluc.mp4", 30, GEOM_B, "frame_{:06d}.jpg", False, set()),
    ("grey.mp4", 20, GEOM_A, "frame_{:06d}.jpg", True, set()),
    ("unpadded.mp4", 12, GEOM_B, "frame_{}.jpg", False, set()),
    ("mixed.mp4", 16, None, "frame_{:06d}.jpg", False, set()),      # frames alternate between the two geometries
]
NO_DIR = "nodir.mp4"
NO_CAPTIONS = "nocaps.mp4"


def build_frames():
    files = {}
    for vi, (video, n, geom, pat, grey, prog) in enumerate(VIDEOS):
        for k in range(1 if pat == "frame_{}.jpg" else 0, n + (1 if pat == "frame_{}.jpg" else 0)):
            h, w = geom if geom is not None else (GEOM_A if k % 2 == 0 else GEOM_B)
            files[f"{video}/{pat.format(k)}"] = jpeg_bytes(frame_pixels(h, w, k, vi + 1, grey), progressive=k in prog)
    return files


def build_gt():
    real = json.load(open(os.path.join(REF, "data/evaluation/formatted_moment_evaluation_gt.json")))
    names = list(real)

    def caps(video, spans):
        src = real[video]["captions"]
        out = []
        for i, (s, e) in enumerate(spans):
            out.append({"start": s, "end": e, "sentence": src[i % len(src)]["sentence"]})
        return {"captions": out, "bounds": [[float(s), float(e)] for s, e in spans]}
    spans = {
        # 40 frames: ordinary spans, a two-frame and a one-frame segment, start == end == 0 (linspace(0, -1) -> index -1 = the last
        # frame), end == n (skipped), end > n (skipped), the progressive frame 17 inside a span
        "nWBuM3LNTcM.mp4": [(0, 6), (6, 8), (8, 9), (0, 0), (14, 18), (21, 39), (30, 40), (35, 52)],
        # 30 frames: start >= n, end > n, a span ending at n - 1, steps sharing frames with their neighbours
        "l2OTMq4aluc.mp4": [(2, 11), (11, 20), (20, 29), (31, 35), (25, 30)],
        "grey.mp4": [(0, 5), (5, 19), (3, 4)],
        # frames 1..12 named without zero padding: index 8 is frame_9.jpg, index 9 frame_10.jpg (lexical order would differ)
        "unpadded.mp4": [(7, 10), (0, 11), (9, 10)],
        "mixed.mp4": [(0, 16), (1, 3), (4, 15)],
        NO_DIR: [(0, 5), (5, 9)],
        NO_CAPTIONS: [],
    }
    src_of = {v: names[i] for i, v in enumerate(spans)}
    src_of["nWBuM3LNTcM.mp4"], src_of["l2OTMq4aluc.mp4"] = "nWBuM3LNTcM.mp4", "l2OTMq4aluc.mp4"
    gt = {v: caps(src_of[v], sp) for v, sp in spans.items()}
    pred = {}
    for v, g in gt.items():
        sents = [c["sentence"] for c in g["captions"]]
        shifted = sents[1:] + sents[:1]                                             # the GT sentences shifted by one step
        pred[v] = {"captions": [{"start": c["start"], "end": c["end"],
                                 "sentence": s.upper() if j % 3 == 0 else (s.title() if j % 3 == 1 else s)}
                                for j, (c, s) in enumerate(zip(g["captions"], shifted))]}
    video_to_cat = {"nWBuM3LNTcM.mp4": "Hobbies and Crafts", "l2OTMq4aluc.mp4": "Hobbies and Crafts", "grey.mp4": "Home and Garden",
                    "unpadded.mp4": "Home and Garden", "mixed.mp4": "Food and Entertaining", NO_DIR: "Health",
                    NO_CAPTIONS: "Pets and Animals",
                    "not_in_gt.mp4": "Sports and Fitness"}                          # a category with no GT video at all
    return gt, pred, video_to_cat


class Recorder:
    def __init__(self, sd, cfg):
        self.sd, self.cfg = sd, cfg
        self.calls = []
        self.pending = None

    def preprocess(self, im):
        self.pending["frames"].append(im.filename)
        return torch.from_numpy(preprocess_cpu.image_transform(np.asarray(im.convert("RGB")), 224))

    def tokenize(self, texts):
        assert len(texts) == 1
        self.pending = {"candidate": texts[0], "frames": []}
        return tokenize(texts, truncate=False)

    def encode_image(self, x):
        return ref_cpu.openai_encode_image(self.sd, x.float(), self.cfg, pip_head=True)

    def encode_text(self, tok):
        return ref_cpu.openai_encode_text(self.sd, tok, self.cfg)


def run_reference(frame_dir, gt, pred, video_to_cat, per_category, rec):
    stubs = {}
    le = types.ModuleType("language_evaluation")

    class CocoEvaluator:
        def run_evaluation(self, cands, refs):
            return {"CIDEr": 0.0}
    le.CocoEvaluator = CocoEvaluator
    stubs["language_evaluation"] = le
    am = types.ModuleType("allennlp_models")
    am.pretrained = types.SimpleNamespace(load_predictor=lambda *a, **k: types.SimpleNamespace(
        predict=lambda premise, hypothesis: {"label_probs": [1.0, 0.0, 0.0]}))
    stubs["allennlp_models"] = am
    bs = types.ModuleType("bert_score")
    bs.score = lambda cands, refs, **k: (torch.zeros(len(cands)),) * 3
    stubs["bert_score"] = bs
    cl = types.ModuleType("clip")
    model = types.SimpleNamespace(encode_image=rec.encode_image, encode_text=rec.encode_text)
    cl.load = lambda name, device=None: (model, rec.preprocess)
    cl.tokenize = rec.tokenize
    stubs["clip"] = cl
    saved = {k: sys.modules.get(k) for k in list(stubs) + ["evaluate"]}
    sys.modules.update(stubs)
    sys.modules.pop("evaluate", None)
    sys.path.insert(0, REF)
    orig_to = torch.Tensor.to

    def to(self, *a, **k):
        if a and isinstance(a[0], str) and a[0].startswith("cuda"):
            return self
        return orig_to(self, *a, **k)

    # torch.mean(dot_score) closes a call: its value is the score the reference appends (float(score.cpu()))
    orig_mean = torch.mean

    def mean(x, *a, **k):
        r = orig_mean(x, *a, **k)
        if not a and not k and x.dim() == 2 and x.shape[1] == 1 and rec.pending is not None:
            rec.pending["score"] = float(r)
            rec.calls.append(rec.pending)
            rec.pending = None
        return r
    try:
        import evaluate as ev
        torch.Tensor.to = to
        torch.mean = mean
        ev.args = types.SimpleNamespace(frame_dir=frame_dir)
        ev.VIDEOS_TO_CAT = video_to_cat
        ev.PROMPT_CATEGORIES = (sorted(set(video_to_cat.values())) + ["all"]) if per_category else ["all"]
        res = ev.evaluate_moment_summarization(gt, pred, 0)
    finally:
        torch.Tensor.to = orig_to
        torch.mean = orig_mean
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return {c: {"CLIPScore": float(r["CLIPScore"]), "Total": int(r["Total"])} for c, r in res.items()}


def to_hf(sd, c):
    """The openai_tiny state dict in transformers' CLIPModel layout."""
    from transformers import CLIPConfig, CLIPModel
    W, T, E = c["vision_width"], c["transformer_width"], c["embed_dim"]
    cfg = CLIPConfig(
        text_config=dict(vocab_size=c["vocab_size"], hidden_size=T, intermediate_size=4 * T, num_hidden_layers=c["transformer_layers"],
                         num_attention_heads=c["transformer_heads"], max_position_embeddings=c["context_length"], hidden_act="quick_gelu",
                         layer_norm_eps=1e-5, eos_token_id=2, projection_dim=E),
        vision_config=dict(hidden_size=W, intermediate_size=4 * W, num_hidden_layers=c["vision_layers"], num_attention_heads=W // 64,
                           image_size=c["image_resolution"], patch_size=c["vision_patch_size"], hidden_act="quick_gelu",
                           layer_norm_eps=1e-5, projection_dim=E),
        projection_dim=E)
    m = CLIPModel(cfg).eval()
    out = {}

    def blocks(src, dst, n, D):
        for i in range(n):
            p, q = f"{src}.resblocks.{i}.", f"{dst}.encoder.layers.{i}."
            w, b = sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"]
            for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
                out[q + f"self_attn.{nm}.weight"] = w[j * D:(j + 1) * D]
                out[q + f"self_attn.{nm}.bias"] = b[j * D:(j + 1) * D]
            for a, b2 in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                          ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
                out[q + b2 + ".weight"] = sd[p + a + ".weight"]
                out[q + b2 + ".bias"] = sd[p + a + ".bias"]
    blocks("visual.transformer", "vision_model", c["vision_layers"], W)
    blocks("transformer", "text_model", c["transformer_layers"], T)
    out.update({
        "vision_model.embeddings.class_embedding": sd["visual.class_embedding"],
        "vision_model.embeddings.patch_embedding.weight": sd["visual.conv1.weight"],
        "vision_model.embeddings.position_embedding.weight": sd["visual.positional_embedding"],
        "vision_model.pre_layrnorm.weight": sd["visual.ln_pre.weight"], "vision_model.pre_layrnorm.bias": sd["visual.ln_pre.bias"],
        "vision_model.post_layernorm.weight": sd["visual.ln_post.weight"], "vision_model.post_layernorm.bias": sd["visual.ln_post.bias"],
        "visual_projection.weight": sd["visual.proj"].t().contiguous(),
        "text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
        "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
        "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
        "text_projection.weight": sd["text_projection"].t().contiguous(),
        "logit_scale": sd["logit_scale"],
    })
    missing, unexpected = m.load_state_dict(out, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    return m


def features(x):
    return x if isinstance(x, torch.Tensor) else x.pooler_output


def main():
    c = synth.OPENAI_VIT_TINY
    sd = synth.openai_clip_state_dict(c, SEED)
    files = build_frames()
    gt, pred, video_to_cat = build_gt()
    tmp = tempfile.mkdtemp()
    try:
        frame_dir = os.path.join(tmp, "frames")
        for rel, data in files.items():
            os.makedirs(os.path.dirname(os.path.join(frame_dir, rel)), exist_ok=True)
            with open(os.path.join(frame_dir, rel), "wb") as f:
                f.write(data)
        runs = {}
        for per_cat in (False, True):
            rec = Recorder(sd, c)
            res = run_reference(frame_dir, gt, pred, video_to_cat, per_cat, rec)
            for call in rec.calls:
                call["frames"] = [os.path.relpath(f, frame_dir) for f in call["frames"]]
            runs["per_category" if per_cat else "all"] = {"result": res, "calls": rec.calls}
            print(("per-category" if per_cat else "all"), json.dumps(res))
        none_res = run_reference("None", gt, pred, video_to_cat, True, Recorder(sd, c))
    finally:
        shutil.rmtree(tmp)
    from hirest_amd import jpeg
    opened = {f for call in runs["all"]["calls"] for f in call["frames"]}
    fallbacks = sorted(rel for rel in opened if not jpeg.parse(files[rel])[0].supported)      # the frames Pillow must decode
    assert fallbacks, "the progressive frame must be one the reference opens"
    # transformers' CLIPModel on the same weights: seeded frames and the candidates' token rows
    hf = to_hf(sd, c)
    img = synth.frames("clipscore.hf.img", (4, 3, 224, 224), SEED + 1)
    tok = tokenize([call["candidate"] for call in runs["all"]["calls"][:5]])
    with torch.no_grad():
        hf_img = features(hf.get_image_features(pixel_values=img)).float()
        hf_txt = features(hf.get_text_features(input_ids=tok)).float()
    orc_img = ref_cpu.openai_encode_image(sd, img, c, pip_head=True)
    orc_txt = ref_cpu.openai_encode_text(sd, tok, c)
    print("transformers vs oracle: image max |diff|", (hf_img - orc_img).abs().max().item(),
          "text max |diff|", (hf_txt - orc_txt).abs().max().item())
    names = sorted(files)
    blob = b"".join(files[n] for n in names)
    offs = np.cumsum([0] + [len(files[n]) for n in names]).astype(np.int64)
    meta = {"seed": SEED, "gt": gt, "pred": pred, "video_to_cat": video_to_cat, "files": names, "fallbacks": fallbacks,
            "runs": runs, "result_no_frames": none_res, "hf_image_frames": "clipscore.hf.img", "hf_image_seed": SEED + 1}
    with open(os.path.join(HERE, "clipscore.json"), "w") as f:
        json.dump(meta, f, indent=1)          # key order is iteration order: not sorted
    np.savez_compressed(os.path.join(HERE, "clipscore.npz"), jpeg_blob=np.frombuffer(blob, np.uint8), jpeg_offsets=offs,
                        hf_tokens=tok.numpy(), hf_image_features=hf_img.numpy(), hf_text_features=hf_txt.numpy())
    # the caption spans of the whole GT split, videos renamed: what tools/clip_score_bench.py shapes its synthetic split after
    real = json.load(open(os.path.join(REF, "data/evaluation/formatted_moment_evaluation_gt.json")))
    spans = [[[d["start"], d["end"]] for d in real[v]["captions"]] for v in real]
    with open(os.path.join(HERE, "clipscore_spans.json"), "w") as f:
        json.dump(spans, f, separators=(",", ":"))
    print(f"{len(names)} frames, {len(blob)} bytes of JPEG, {len(runs['all']['calls'])} scored captions, fallbacks {fallbacks}")


if __name__ == "__main__":
    main()
