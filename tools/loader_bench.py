#!/usr/bin/env python3
"""Loader throughput of the joint model: the device loader (hirest_amd/dataset.py + csrc/batch.hip) next to the host path that
existed before it — per sample ``features.load_video_features`` + ``features.fit_asr``, stack, ``.to(device)`` — in one process
and with 4 ``DataLoader`` workers as the reference configures (args.py: --num_workers 4).

A synthetic corpus with HiREST-like lengths (1-10 minute videos at one feature row per second, a subtitle every ~5 s) is written
to a temporary directory.  For B in {5, 32} at n_model_frames = 300 and -1 it prints batches/s of every loader, the assemble
kernel's write rate as a fraction of the plain-copy rate of DESIGN 4.1, and the wall time per batch of moment retrieval and of a
training step (forward + backward) fed by either loader.  One JSON object per line.

    python tools/loader_bench.py [--videos 256] [--batches 40]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hirest_amd  # noqa: E402
from hirest_amd import dataset as ds, features, synth  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s of a plain device copy (read + write), DESIGN 4.1
D, DA = 1024, 384


def write_corpus(root, n_videos, seed=0):
    rng = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    for sub in ("feats", "srt", "asr"):
        os.makedirs(os.path.join(root, sub))
    split = {}
    stamp = lambda s: f"{s // 3600:02d}:{s // 60 % 60:02d}:{s % 60:02d},000"
    for v in range(n_videos):
        n = int(rng.randint(60, 601))
        name = f"video{v:04d}.mp4"
        torch.save(torch.randn(n, D, generator=gen), os.path.join(root, "feats", f"{name}.pt"))
        starts = np.sort(rng.choice(n, size=max(1, n // 5), replace=False))
        spans = [(int(s), int(min(n, s + rng.randint(1, 7)))) for s in starts]
        torch.save(torch.randn(len(spans), DA, generator=gen), os.path.join(root, "asr", f"video{v:04d}.pt"))
        with open(os.path.join(root, "srt", f"video{v:04d}.srt"), "w") as f:
            f.write("".join(f"{i + 1}\n{stamp(s)} --> {stamp(e)}\nwords\n\n" for i, (s, e) in enumerate(spans)))
        a, b = sorted(rng.randint(0, n, size=2).tolist())
        split.setdefault(f"prompt number {v // 2}", {})[name] = {"relevant": True, "clip": True, "v_duration": float(n), "bounds": [a, b], "steps": []}
    json.dump(split, open(os.path.join(root, "all_data_test.json"), "w"))


class HostDataset(torch.utils.data.Dataset):
    """The host path of the parent commit: the row rules of hirest_amd/features.py per sample, the reference's collate."""

    def __init__(self, d: ds.MomentDataset):
        self.d = d

    def __len__(self):
        return len(self.d)

    def __getitem__(self, i):
        e, F = self.d.data[i], self.d.n_model_frames
        vis = features.load_video_features(self.d.video_feature_dir / f"{e['fname']}.pt", F, "dataset")
        vid = e["fname"].replace(".mp4", "")
        asr = features.fit_asr(torch.load(self.d.asr_feature_dir / f"{vid}.pt", map_location="cpu"), self.d.videoid2asr[vid], vis, F)
        return {"vis": vis.float(), "asr": asr, "mask": self.d.moment_mask(i), "start": e["moment_retrieval_start_target"],
                "end": e["moment_retrieval_end_target"], "prompt": e["prompt"]}

    @staticmethod
    def collate(items):
        T = max(x["vis"].shape[0] for x in items)
        pad = lambda t: torch.cat([t, torch.zeros((T - t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype)])
        return {"tasks": ["moment_retrieval"] * len(items), "vis_feats": torch.stack([pad(x["vis"]) for x in items]),
                "asr_feats": torch.stack([pad(x["asr"]) for x in items]),
                "vis_mask": torch.stack([pad(torch.ones(x["vis"].shape[0], dtype=torch.long)) for x in items]),
                "moment_mask": torch.stack([pad(x["mask"]) for x in items]),
                "moment_retrieval_start_target": torch.tensor([x["start"] for x in items]),
                "moment_retrieval_end_target": torch.tensor([x["end"] for x in items]),
                "clip_text_ids": hirest_amd.tokenize([x["prompt"] for x in items])}


def to_device(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def timed(make_iter, n, dev, consume=None):
    """Seconds per batch over n batches of a fresh iterator (the first batch, which starts workers, is not timed)."""
    it = make_iter()
    first = next(it)
    if consume:
        consume(first)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    k = 0
    for batch in it:
        if consume:
            consume(batch)
        k += 1
        if k == n:
            break
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / max(k, 1), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=256)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--no-model", action="store_true", help="loader rates only")
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="hirest_loader_bench_")
    write_corpus(root, opt.videos)
    model = None
    if not opt.no_model:
        shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(REPO, "tests", "golden", "joint_schema.json"))).items()}
        model = hirest_amd.MomentModel(n_frames=-1, asr_dim=DA, args=None, clip_model=None)
        model.load_state_dict(synth.joint_state_dict(shapes, 31), strict=False)
        model = model.to(dev).eval()
    slower = []
    for F in (300, -1):
        args = types.SimpleNamespace(data_dir=root, video_feature_dir=os.path.join(root, "feats"), asr_dir=os.path.join(root, "srt"),
                                     asr_feature_dir=os.path.join(root, "asr"), n_model_frames=F, distributed=False, end_to_end=False)
        for B in (5, 32):
            t0 = time.perf_counter()
            loader = ds.get_moment_loader(args, "test", B, "moment_retrieval", device=dev)
            torch.cuda.synchronize(dev)
            build_s = time.perf_counter() - t0
            n = min(opt.batches, len(loader) - 1)
            host = HostDataset(loader.dataset)
            text = torch.randn(B, 1024, generator=torch.Generator().manual_seed(1)).to(dev)

            def host_iter(workers):
                dl = torch.utils.data.DataLoader(host, batch_size=B, shuffle=False, num_workers=workers, pin_memory=True, collate_fn=host.collate)
                return (to_device(b, dev) for b in dl)
            res = {"n_model_frames": F, "B": B, "videos": opt.videos, "batches_timed": n, "store_build_s": round(build_s, 3),
                   "store_MB": round(loader.tables.store.nbytes / 1e6, 1)}
            for name, make in (("device", lambda: iter(loader)), ("host_1proc", lambda: host_iter(0)), ("host_4workers", lambda: host_iter(4))):
                s, k = timed(make, n, dev)
                res[f"{name}_batches_per_s"] = round(1.0 / s, 1)
                res[f"{name}_us_per_batch"] = round(s * 1e6, 1)
            # the kernel alone: device time of the launches between two events, bytes written per second
            order = torch.arange(B, dtype=torch.int32, device=dev)
            batch = loader.tables.assemble(order, list(range(B)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 50
            e0.record()
            for _ in range(reps):
                batch = loader.tables.assemble(order, list(range(B)))
            e1.record()
            torch.cuda.synchronize(dev)
            written = sum(batch[k].numel() * batch[k].element_size() for k in ("vis_feats", "asr_feats", "vis_mask", "moment_mask"))
            us = e0.elapsed_time(e1) * 1e3 / reps
            res["assemble_us_back_to_back"] = round(us, 2)
            res["assemble_bytes_written"] = written
            res["assemble_write_TBps"] = round(written / us / 1e6, 3)
            res["assemble_fraction_of_copy_rate"] = round(2 * written / (us * 1e-6) / COPY_RATE, 3)      # a copy reads what it writes
            if model is not None:
                def feed(step):
                    def consume(b):
                        b = dict(b, text_feat=text[:b["vis_feats"].shape[0]])
                        step(b)
                    return consume

                def retrieval(b):
                    model.test_step(b)

                def train(b):
                    model.train_step(b)["loss"].backward()
                for what, step in (("retrieval", retrieval), ("train_step", train)):
                    for name, make in (("device", lambda: iter(loader)), ("host_1proc", lambda: host_iter(0)), ("host_4workers", lambda: host_iter(4))):
                        s, k = timed(make, min(n, 20), dev, feed(step))
                        res[f"{what}_ms_per_batch_fed_by_{name}"] = round(s * 1e3, 3)
            res["device_not_slower_than_host"] = bool(res["device_batches_per_s"] >= max(res["host_1proc_batches_per_s"], res["host_4workers_batches_per_s"]))
            print(json.dumps(res), flush=True)
            slower += [] if res["device_not_slower_than_host"] else [(F, B)]
    if slower:
        print(f"FAILED: the device loader is slower than the host path at (n_model_frames, B) = {slower}", flush=True)
        sys.exit(1)
    print("OK: the device loader is not slower than the host path (one process or 4 workers) at any configuration", flush=True)


if __name__ == "__main__":
    main()
