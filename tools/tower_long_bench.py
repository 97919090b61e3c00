#!/usr/bin/env python3
"""Frames/s of a synthetic ViT-L/14@336px vision tower (24 layers, width 1024, 16 heads of 64, 577 tokens) per precision, at --frames
frames per encode_image call.  'bf16' runs the streaming attention (csrc/attention_long.hip); CLIP.set_precision maps 'bf16x3' to
the exact-fp32 kernels for this tower, so that figure is what the shape had to run on before."""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hirest_amd import clip, synth  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--precisions", nargs="*", default=["bf16", "bf16x3"])
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg = {"embed_dim": 768, "image_resolution": 336, "vision_layers": 24, "vision_width": 1024, "vision_patch_size": 14,
       "context_length": 77, "vocab_size": 512, "transformer_width": 128, "transformer_heads": 2, "transformer_layers": 1}
model = clip.build_model(synth.openai_clip_state_dict(cfg, 7)).to(dev)
model.visual.pip_head = True
img = torch.randn((a.frames, 3, 336, 336), device=dev)
for precision in a.precisions:
    model.set_precision(precision)
    iters = a.iters if precision == "bf16" else max(2, a.iters // 5)
    for _ in range(2):
        out = model.encode_image(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = model.encode_image(img)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"ViT-L/14@336px tower, precision {precision} (kernels: {model.visual.precision}): {a.frames} frames per call, {dt * 1e3:.1f} ms per call, "
          f"{a.frames / dt:.0f} frames/s, finite {bool(torch.isfinite(out).all())}", flush=True)
