#!/usr/bin/env python3
"""End-to-end cascade (hirest_amd.cascade.run_end_to_end) against three chained MomentModel.test_step calls with host-built
batches between them (what a user of the per-task API has to write: the dataset's rules of hirest_dataset.py:250-261, :285-304
in Python), on the same in-memory loader batch.  B = 5 and B = 32, T = 300, beam 5, fp32 and bf16x3.  Prints videos/s as the
median of the timed repeats with their spread, the per-stage times of the chain and the split of the cascade into
(retrieval + segmentation + seams) and captioning.

    python tools/cascade_bench.py [--repeats 7] [--out profiles/r07/cascade.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hirest_amd  # noqa: E402
from hirest_amd import cascade, synth  # noqa: E402
from hirest_amd.timeline import frame_index_to_timestamp, timestamp_to_frame_index  # noqa: E402

T, BEAMS = 300, 5


def chain(model, batch, durations, stages=None):
    """Three test_step calls; the batches between them are built on the host."""
    def tick(name, t0):
        if stages is not None:
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()
    B = batch["vis_mask"].shape[0]
    t0 = time.perf_counter()
    pred = model.test_step(dict(batch, tasks=["moment_retrieval"]))["prediction"]
    t0 = tick("retrieval", t0)
    ts = [[frame_index_to_timestamp(f, durations[b], T) for f in pred[b]] for b in range(B)]
    bf = [[timestamp_to_frame_index(t, durations[b], T) for t in ts[b]] for b in range(B)]
    t0 = tick("seam a (host)", t0)
    seg = model.test_step(dict(batch, tasks=["moment_segmentation"], moment_bound_frames=torch.tensor(bf)))["prediction"]
    t0 = tick("segmentation", t0)
    rows, masks, step_ts = [], [], []
    for b in range(B):
        st = [[frame_index_to_timestamp(seg[b][j], durations[b], T), frame_index_to_timestamp(seg[b][j + 1], durations[b], T)]
              for j in range(len(seg[b]) - 1)]
        step_ts.append(st)
        for s0, s1 in st:
            a, e = timestamp_to_frame_index(s0, durations[b], T), timestamp_to_frame_index(s1, durations[b], T)
            m = torch.zeros(T, dtype=torch.long)
            m[a:e] = 1
            m[e] = 1
            masks.append(m)
            rows.append(b)
    t0 = tick("seam b (host)", t0)
    ids = []
    if rows:
        r = torch.tensor(rows)
        cap = {"tasks": ["step_captioning"], "vis_feats": batch["vis_feats"][r], "asr_feats": batch["asr_feats"][r],
               "moment_mask": torch.stack(masks), "text_feat": batch["text_feat"][r]}
        t0 = tick("seam c (host: S-fold feature copy)", t0)
        ids = model.test_step(cap, num_beams=BEAMS, return_ids=True)["token_ids"]
        t0 = tick("captioning", t0)
    return pred, seg, step_ts, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(here, "..", "tests", "golden", "joint_schema.json"))).items()}
    sd = synth.joint_state_dict(shapes, 31)
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5
    dev = torch.device("cuda:0")
    model = hirest_amd.MomentModel(n_frames=T, asr_dim=384, args=None, clip_model=None)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"cascade_bench: T = {T}, beam {BEAMS}, median of {a.repeats} timed repeats after 2 warm-up runs; {torch.cuda.get_device_name(0)}")
    for precision in ("fp32", "bf16x3"):
        model.set_precision(precision)
        for B in (5, 32):
            vis, asr, text, vis_mask, moment_mask, _ = synth.joint_inputs(f"cascade.bench.{B}", B, T, 43)
            durations = [200 + (37 * b) % 700 for b in range(B)]
            batch = {"vis_feats": vis, "asr_feats": asr, "text_feat": text, "vis_mask": torch.ones_like(vis_mask),
                     "moment_mask": torch.ones_like(moment_mask), "video_duration": durations}
            res = {}
            for name, fn in (("chain", lambda: chain(model, batch, durations)),
                             ("cascade", lambda: cascade.run_end_to_end(model, [batch], num_beams=BEAMS, return_ids=True))):
                for _ in range(2):
                    out = fn()
                times = []
                for _ in range(a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                res[name] = (times, out)
            c_out, e_out = res["chain"][1], res["cascade"][1][0]
            same = (c_out[0] == e_out["moment_frames"] and c_out[1] == e_out["boundary_frames"] and c_out[2] == e_out["step_bounds"]
                    and c_out[3] == [c for caps in e_out["captions"] for c in caps])
            S = len(c_out[3])
            say(f"\n{precision} B = {B}: {S} steps captioned; results equal: {same}")
            for name in ("chain", "cascade"):
                t = sorted(res[name][0])
                med = statistics.median(t)
                say(f"  {name:8s} {B / med:8.2f} videos/s   median {med * 1e3:8.2f} ms   min {t[0] * 1e3:8.2f}   max {t[-1] * 1e3:8.2f}   "
                    f"spread {(t[-1] - t[0]) / med * 100:5.1f} %")
            mc, me = statistics.median(res["chain"][0]), statistics.median(res["cascade"][0])
            say(f"  cascade / chain time: {me / mc:.3f}")
            stages = {}
            for _ in range(3):
                chain(model, batch, durations, stages)
            say("  chain by stage (synchronised after each, mean of 3): " +
                ", ".join(f"{k} {v / 3 * 1e3:.2f} ms" for k, v in stages.items()))
            t12 = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad(), torch.cuda.device(dev):
                    cascade._stages(model, batch)
                torch.cuda.synchronize()
                t12.append(time.perf_counter() - t0)
            say(f"  cascade: retrieval + segmentation + seams a, b, c {statistics.mean(t12) * 1e3:.2f} ms, "
                f"captioning + read-out {(me - statistics.mean(t12)) * 1e3:.2f} ms (by difference)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
