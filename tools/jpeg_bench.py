#!/usr/bin/env python3
"""Device JPEG decode throughput next to Pillow on a 16-thread pool, and extract_frame_dir end to end next to the tower alone.

Inputs: deterministic synthetic frames encoded by Pillow at q95 4:2:0 (what extract_frames.py's cv2.imwrite writes) at 360p,
720p and 1080p in two content levels: "blocky" (synth.rgb_frames: flat 8x8 blocks, half with per-pixel noise; large files)
and "smooth" (a gradient with mild noise; small files).  Entropy decode time scales with the compressed bytes, so both are
reported.  Both entropy modes ("lanes": one lane per image; "chunked": a workgroup of lanes per image) are timed in this one
process, alternating call by call, at every --batches size; the per-image chunk sizes, lanes and sync rounds of the chunked
mode come from Decoder.chunk_info().  Prints one JSON line."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from PIL import Image  # noqa: E402

from hirest_amd import features, jpeg, synth  # noqa: E402

GEOMS = {"360p": (360, 640), "720p": (720, 1280), "1080p": (1080, 1920)}


def encode(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=95, subsampling=2)
    return b.getvalue()


def frames(level, h, w, n):
    if level == "blocky":
        return synth.rgb_frames(f"jpegbench.{h}", (n, h, w, 3), 1)
    rng = np.random.default_rng(h)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        g = np.stack([(x + 13 * i) * 255 // w, y * 255 // h, (x + y + 29 * i) * 255 // (w + h)], -1)
        out.append((g + rng.integers(-4, 5, (h, w, 3))).clip(0, 255).astype(np.uint8))
    return np.stack(out)


def pillow_decode(b):
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def alternating(fns, iters):
    """{name: [seconds per call]}: the calls of the different names alternate, so drift of the box hits them alike."""
    out = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            out[k].append(timed(fn, 1))
    return out


def spread(v):
    return {"min": round(float(np.min(v)), 2), "median": round(float(np.median(v)), 2), "max": round(float(np.max(v)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,256,4", help="frames per device decode call, comma-separated")
    ap.add_argument("--entropy", default="lanes,chunked", help="entropy modes to time, comma-separated")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16, help="distinct encoded frames (repeated to fill a batch)")
    ap.add_argument("--pillow-frames", type=int, default=256)
    ap.add_argument("--extract-frames", type=int, default=1024, help="1080p frames through extract_frame_dir (0: skip)")
    ap.add_argument("--geoms", default="360p,720p,1080p")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    modes = a.entropy.split(",")
    batches = [int(b) for b in a.batches.split(",")]
    decoders = {m: jpeg.Decoder(entropy=m) for m in modes}
    res = {"decode": {}, "modes": modes, "iters": a.iters}
    pool = ThreadPoolExecutor(max_workers=jpeg.IO_THREADS)
    blobs_1080 = {}
    for g in a.geoms.split(","):
        h, w = GEOMS[g]
        for level in ("blocky", "smooth"):
            distinct = [encode(f) for f in frames(level, h, w, a.distinct)]
            if g == "1080p":
                blobs_1080[level] = distinct
            pb = [distinct[i % len(distinct)] for i in range(a.pillow_frames)]
            list(pool.map(pillow_decode, pb[:32]))
            t0 = time.perf_counter()
            list(pool.map(pillow_decode, pb))
            sp = time.perf_counter() - t0
            row = {"bytes_per_frame": round(sum(len(b) for b in distinct) / len(distinct)), "pillow16_frames_per_s": round(len(pb) / sp, 1)}
            for nb in batches:
                batch = [distinct[i % len(distinct)] for i in range(nb)]
                nbytes = sum(len(b) for b in batch)
                ref = None
                for m in modes:                                      # warm-up (allocations, first launch) and the same-bits check
                    out = decoders[m].decode(batch, dev)
                    assert not decoders[m].last_fallbacks, decoders[m].last_fallbacks
                    ref = out.clone() if ref is None else ref
                    assert torch.equal(out, ref), (g, level, nb, m)
                del ref, out
                if "chunked" in modes and "chunks" not in row:
                    info = decoders["chunked"].chunk_info()
                    row["chunks"] = {"chunk_bytes": spread(info[:, 0]), "lanes": spread(info[:, 1]), "sync_rounds": spread(info[:, 2])}
                secs = alternating({m: (lambda m=m: decoders[m].decode(batch, dev)) for m in modes}, a.iters)
                for m in modes:
                    s = float(np.median(secs[m]))
                    row[f"{m}_b{nb}"] = {"frames_per_s": round(nb / s, 1), "compressed_MB_per_s": round(nbytes / s / 1e6, 1),
                                        "over_pillow16": round((nb / s) / (len(pb) / sp), 2),
                                        "seconds_per_call": [round(x, 4) for x in secs[m]]}
            res["decode"][f"{g}_{level}"] = row
            print(g, level, row, file=sys.stderr, flush=True)
    if a.extract_frames > 0 and blobs_1080:
        import hirest_amd
        model = hirest_amd.EVA_CLIP(**synth.EVA_CLIP_G_14).to(dev).eval()
        model.init_random_(seed=1234)
        tmp = tempfile.mkdtemp(prefix="jpegbench")
        try:
            for level in ("blocky", "smooth"):
                src = os.path.join(tmp, level, "frames")
                per_video = 256
                n_vid = max(1, a.extract_frames // per_video)
                for v in range(n_vid):
                    d = os.path.join(src, f"video{v}")
                    os.makedirs(d)
                    for t in range(per_video):
                        with open(os.path.join(d, f"frame_{t}.jpg"), "wb") as f:
                            f.write(blobs_1080[level][(t + v) % len(blobs_1080[level])])
                out = os.path.join(tmp, level, "out")
                n = n_vid * per_video
                ends = {}
                for m in modes:                       # extract_frame_dir takes the module's decoder: the environment picks its mode
                    os.environ["HIREST_JPEG_ENTROPY"] = m
                    features.extract_frame_dir(model, src, out)                   # warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    features.extract_frame_dir(model, src, out)
                    torch.cuda.synchronize()
                    ends[m] = time.perf_counter() - t0
                os.environ.pop("HIREST_JPEG_ENTROPY")
                # the tower alone on the same decoded frames (device preprocess + encode, no decode, no files)
                dec = [jpeg.read_frame_dir(os.path.join(src, f"video{v}"), dev, entropy=modes[-1]) for v in range(n_vid)]
                features.frame_features_many(model, dec)
                st = timed(lambda: features.frame_features_many(model, dec), 1)
                res[f"extract_frame_dir_1080p_{level}"] = {"frames": n, "tower_only_frames_per_s": round(n / st, 1)}
                for m in modes:
                    res[f"extract_frame_dir_1080p_{level}"][m] = {"end_to_end_frames_per_s": round(n / ends[m], 1),
                                                                  "ratio": round(st / ends[m], 3)}
                print(level, res[f"extract_frame_dir_1080p_{level}"], file=sys.stderr, flush=True)
                del dec
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
