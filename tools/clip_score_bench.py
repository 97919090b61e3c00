#!/usr/bin/env python3
"""CLIPScore over a synthetic split shaped like the reference's step-captioning GT (evaluate.py:190-320), end to end.

The split: the 507 videos and 3 856 caption spans of formatted_moment_evaluation_gt.json (tests/golden/clipscore_spans.json),
each video with as many frames as its last ``end`` (so its last caption is skipped, as in the real data), every 25th video cut
to half its length so that more skips occur.  Frames are 360p (``--res 720p``) q95 4:2:0 JPEGs: ``--distinct`` encoded frames,
half smooth and half blocky (tools/jpeg_bench.py's content), hard-linked under every frame name, so the set-up is quick and
the decode sees realistic sizes.  The model is ViT-B/32-shaped with random weights (width 768, 12 layers, embed 512, 224 px)
and the pip CLS head.

Prints one JSON line: captions/s end to end, the unique frames decoded, the seconds of each stage (from a second run that
synchronises after each stage), and the reference's way for comparison: one caption at a time, four frames decoded by Pillow,
the tower on 4 frames and the text tower on 1 (device preprocess and the scoring kernel), timed on ``--loop-sample`` captions
and scaled to the split."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from PIL import Image  # noqa: E402

from hirest_amd import clip, evaluation, jpeg, ops, synth  # noqa: E402
from hirest_amd.features import _prepare_frames  # noqa: E402
from hirest_amd.tokenizer import tokenize  # noqa: E402

GEOMS = {"360p": (360, 640), "720p": (720, 1280)}
WORDS = "take the cut add glue fold paper stitch cloth mix flour pour water open lid attach wheel tighten screw".split()


def encode(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=95, subsampling=2)
    return b.getvalue()


def pool_frames(h, w, n):
    rng = np.random.default_rng(h)
    y, x = np.mgrid[0:h, 0:w]
    blocky = synth.rgb_frames(f"clipscorebench.{h}", (n - n // 2, h, w, 3), 1)
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append(np.asarray(blocky[i // 2]))
        else:
            g = np.stack([(x + 13 * i) * 255 // w, y * 255 // h, (x + y + 29 * i) * 255 // (w + h)], -1)
            out.append((g + rng.integers(-4, 5, (h, w, 3))).clip(0, 255).astype(np.uint8))
    return out


def build_split(root, res, distinct):
    with open(os.path.join(REPO, "tests", "golden", "clipscore_spans.json")) as f:
        spans = json.load(f)
    h, w = GEOMS[res]
    pool_dir = os.path.join(root, "pool")
    os.makedirs(pool_dir)
    pool = []
    for i, a in enumerate(pool_frames(h, w, distinct)):
        p = os.path.join(pool_dir, f"p{i}.jpg")
        with open(p, "wb") as f:
            f.write(encode(a))
        pool.append(p)
    frame_dir = os.path.join(root, "frames")
    gt, pred = {}, {}
    rng = np.random.default_rng(0)
    k = 0
    for v, sp in enumerate(spans):
        video = f"video{v:03d}.mp4"
        n = max([e for _, e in sp] + [0])
        if v % 25 == 0:
            n //= 2
        d = os.path.join(frame_dir, video)
        os.makedirs(d)
        for t in range(n):
            os.link(pool[k % len(pool)], os.path.join(d, f"frame_{t:06d}.jpg"))
            k += 1
        gt[video] = {"captions": [{"start": s, "end": e, "sentence": ""} for s, e in sp]}
        pred[video] = {"captions": [{"sentence": " ".join(rng.choice(WORDS, int(rng.integers(2, 8))))} for _ in sp]}
    return frame_dir, gt, pred, sum(os.path.getsize(p) for p in pool) / len(pool)


def reference_loop(model, plan, sample, dev):
    """evaluate.py:235-262 driven as the reference drives it: per caption, Pillow decodes 4 frames, one tower call on 4 frames, one
    text call on 1 candidate, one score read back."""
    picks = np.linspace(0, len(plan.scored) - 1, min(sample, len(plan.scored))).astype(int)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in picks:
        files = [plan.frames[r] for r in plan.sel[j]]
        u8 = torch.from_numpy(np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])).to(dev)
        img = model.encode_image(_prepare_frames(model, u8)).contiguous()
        txt = model.encode_text(tokenize([plan.candidates[plan.scored[j]]]).to(dev))
        float(ops.clip_score(img, txt, torch.arange(4, dtype=torch.int32).reshape(1, 4)).cpu())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(picks), len(picks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="360p", choices=sorted(GEOMS))
    ap.add_argument("--distinct", type=int, default=256, help="distinct encoded frames behind the hard links")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--loop-sample", type=int, default=200, help="captions timed the reference's way (0: skip)")
    ap.add_argument("--chunk", type=int, default=evaluation.CLIP_SCORE_CHUNK)
    ap.add_argument("--tmp", default=None, help="directory for the synthetic frames (default: a new temporary directory)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="clipscorebench", dir=a.tmp)
    try:
        t0 = time.perf_counter()
        frame_dir, gt, pred, bytes_per_frame = build_split(root, a.res, a.distinct)
        setup_s = time.perf_counter() - t0
        ckpt = os.path.join(root, "b32.pt")
        torch.save(synth.openai_clip_state_dict(synth.OPENAI_VIT_B32, 1), ckpt)
        model, _ = clip.load(ckpt, device=dev, pip_head=True, precision=a.precision)
        t0 = time.perf_counter()
        plan = evaluation.clip_score_plan(gt, pred, frame_dir)
        plan_s = time.perf_counter() - t0
        warm = evaluation.clip_score_plan(gt, pred, frame_dir, videos=list(gt)[:20])
        evaluation._plan_scores(warm, model, dev, chunk=a.chunk)                  # warm-up: allocations, first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = evaluation._plan_scores(plan, model, dev, chunk=a.chunk)
        torch.cuda.synchronize()
        pipe_s = time.perf_counter() - t0
        stats = {}
        evaluation._plan_scores(plan, model, dev, chunk=a.chunk, stats=stats)    # the same run, synchronised per stage
        blobs = jpeg._pool_map(jpeg._read, plan.frames[:1024])
        t0 = time.perf_counter()
        for b in blobs:
            jpeg.parse(b)
        parse_s = (time.perf_counter() - t0) * len(plan.frames) / len(blobs)
        total_s = plan_s + pipe_s
        res = {"res": a.res, "precision": a.precision, "videos": len(gt), "captions": len(plan.captions), "scored": len(plan.scored),
               "unique_frames": len(plan.frames), "bytes_per_frame": round(bytes_per_frame), "chunk": a.chunk,
               "setup_s": round(setup_s, 2), "plan_s": round(plan_s, 3), "pipeline_s": round(pipe_s, 3), "total_s": round(total_s, 3),
               "captions_per_s": round(len(plan.captions) / total_s, 1),
               "stages_s": {k: round(v, 3) for k, v in stats.items() if k.endswith("_s")},
               "host_parse_s_within_decode": round(parse_s, 3), "fallbacks": len(stats["fallbacks"]),
               "mean_score": float(np.mean(scores))}
        if a.loop_sample > 0:
            reference_loop(model, plan, 4, dev)                                       # warm-up
            per, n = reference_loop(model, plan, a.loop_sample, dev)
            res["reference_way"] = {"sampled_captions": int(n), "s_per_caption": round(per, 5),
                                    "scaled_s": round(per * len(plan.scored), 2),
                                    "note": "timed on the sample, scaled to the split's scored captions",
                                    "speedup": round(per * len(plan.scored) / total_s, 2)}
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
