#!/usr/bin/env python3
"""One validation batch (run.py:546-571), two ways on the same machine and model:

  two calls   ``train_step(batch)`` under ``eval()`` / ``no_grad``, then ``test_step(batch)`` — the hand-written loop around this
              package's steps, which is all there was before ``valid_step``;
  valid_step  ``MomentModel.valid_step(batch)``: loss and prediction from one forward.

Operating points: moment retrieval at B = 5 and B = 32, T = 300; step captioning at B = 5 and B = 32, beam 5; fp32 and bf16x3.
Five runs per point; the two arms alternate their order from run to run; a run times `--reps` back-to-back batches per arm with one
synchronisation at the end.  Reported: the median of the five runs per arm, and the spread (max - min) of the two-call arm's runs.
Also the peak device allocation of ONE captioning batch at B = 32 per arm.

    python tools/valid_bench.py [--reps 10] [--out profiles/valid/ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hirest_amd  # noqa: E402
from hirest_amd import synth  # noqa: E402
from hirest_amd.synth import joint_inputs, train_targets, caption_targets  # noqa: E402


def batches_for(B, T):
    vis, asr, text, vis_mask, moment_mask, bounds = joint_inputs(f"vb.{B}.{T}", B, T, 67)
    st, et, _, _ = train_targets(f"vb.{B}.{T}", B, T, 67, bounds)
    cap_mask = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        cap_mask[b, 10 + b:10 + b + [15, 7, 20, 37, 12, 25, 3, 18][b % 8]] = 1
    common = {"vis_feats": vis, "vis_mask": vis_mask, "asr_feats": asr, "text_feat": text}
    out = {"moment_retrieval": dict(common, tasks=["moment_retrieval"] * B, moment_mask=moment_mask, moment_retrieval_start_target=st,
                                    moment_retrieval_end_target=et),
           "step_captioning": dict(common, tasks=["step_captioning"] * B, moment_mask=cap_mask,
                                   target_text=caption_targets(f"vb.{B}.{T}", B, 48, 67))}
    # pinned, as DataLoader(pin_memory=True) delivers them (hirest_dataset.py:614,624)
    return {k: {n: (v.pin_memory() if isinstance(v, torch.Tensor) else v) for n, v in b.items()} for k, b in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valid", "ab.json"))
    a = ap.parse_args()
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "joint_schema.json"))).items()}
    sd = synth.joint_state_dict(shapes, 31)
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5          # some beams end early, as in the caption fixtures
    dev = torch.device("cuda:0")
    model = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=None, clip_model=None)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "runs": a.runs, "points": []}
    data = {B: batches_for(B, 300) for B in (5, 32)}
    for precision in ("fp32", "bf16x3"):
        model.set_precision(precision)
        for task, kw in (("moment_retrieval", {}), ("step_captioning", {"num_beams": 5})):
            for B in (5, 32):
                batch = data[B][task]

                def two_calls():
                    with torch.no_grad():
                        loss = model.train_step(batch)["loss"]
                    return loss, model.test_step(batch, **kw)

                def valid():
                    r = model.valid_step(batch, **kw)
                    return r["loss"], r
                arms = {"two_calls": two_calls, "valid_step": valid}
                for fn in arms.values():
                    fn(); fn()
                torch.cuda.synchronize()
                times = {k: [] for k in arms}
                for run in range(a.runs):
                    for name in (list(arms) if run % 2 == 0 else list(arms)[::-1]):
                        t0 = time.perf_counter()
                        for _ in range(a.reps):
                            arms[name]()
                        torch.cuda.synchronize()
                        times[name].append((time.perf_counter() - t0) / a.reps * 1e3)
                point = {"precision": precision, "task": task, "B": B, "T": 300,
                         "two_calls_ms": statistics.median(times["two_calls"]), "valid_step_ms": statistics.median(times["valid_step"]),
                         "two_calls_spread_ms": max(times["two_calls"]) - min(times["two_calls"]), "runs_ms": times}
                if task == "step_captioning" and B == 32:
                    for name, fn in arms.items():
                        torch.cuda.synchronize()
                        level = torch.cuda.memory_allocated(dev)
                        torch.cuda.reset_peak_memory_stats(dev)
                        fn()
                        torch.cuda.synchronize()
                        point[f"{name}_peak_bytes"] = torch.cuda.max_memory_allocated(dev)
                        point[f"{name}_peak_above_level_bytes"] = torch.cuda.max_memory_allocated(dev) - level
                result["points"].append(point)
                print(f"[{precision}] {task} B={B}: two calls {point['two_calls_ms']:.2f} ms (spread {point['two_calls_spread_ms']:.2f}), "
                      f"valid_step {point['valid_step_ms']:.2f} ms" +
                      (f", peak above level {point['two_calls_peak_above_level_bytes'] / 2**20:.0f} -> "
                       f"{point['valid_step_peak_above_level_bytes'] / 2**20:.0f} MiB" if "valid_step_peak_bytes" in point else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
