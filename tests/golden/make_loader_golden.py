#!/usr/bin/env python3
"""Generate tests/golden/loader_a.{npz,json}: the REAL reference's loader (hirest_dataset.py) on a small throw-away data directory.

Runs only where the reference checkout is available (see make_golden.py, whose stubs it reuses, and make_cascade_golden.py, whose
BertTokenizer stand-in it reuses).  What runs is the reference's own ``MomentDataset`` constructor, ``__getitem__`` and
``collate_fn`` — for the three tasks, both segmentation paths (``all_data_train.json`` / ``all_data_test.json``),
``n_model_frames`` in {-1, 8, 48} and batch sizes 1 and 3 — and its ``MultitaskLoader``.  The ``srt`` package is not installed
offline: the stub module gets a ``parse`` that reads the timing lines of the transcripts written here into ``timedelta`` pairs,
which is all the reference uses of a subtitle (``sub.start.seconds`` / ``sub.end.seconds``).

Stored: the inputs (the split, the transcripts and MultitaskLoader's task orders in loader_a.json; the feature arrays with D = 16 /
Da = 8 in loader_a.npz) and, per configuration, every scalar of every example with its masks as lists, and every tensor and list of
every collated batch in sequential order (tensors as npz arrays, the rest as JSON text in the npz entry ``configs.json``).

    python tests/golden/make_loader_golden.py
"""
import datetime
import json
import os
import re
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository on sys.path)
from make_cascade_golden import _Tok  # noqa: E402

D, DA, MAX_WORDS = 16, 8, 12
# rows of the feature file, v_duration (round() gives the row count: 30.5 and 47.5 are ties that round down and up)
VIDEOS = {"v5.mp4": (5, 4.6), "v30.mp4": (30, 30.5), "v8.mp4": (8, 8.4), "v95.mp4": (95, 95.4), "v48.mp4": (48, 47.5),
          "nosteps.mp4": (12, 12.2), "onestep.mp4": (30, 29.7)}
# subtitles (start, end) in seconds; ASR feature rows = subtitles (+ EXTRA_ASR_ROWS unused rows)
SUBS = {"v5": [],                                                     # a transcript without subtitles
        "v30": [(2.0, 10.5), (8.2, 12.0), (20.9, 22.1)],              # two overlap: the later one wins on 8 .. 9
        "v8": [(3.1, 3.9), (6.0, 20.0), (1.0, 2.999)],                # start == end in whole seconds; one runs past the end
        "v95": [(1.0, 3.0), (10.0, 20.0), (95.0, 99.0), (100.0, 120.0), (3599.0, 3605.5)],   # at / after the end; an hour field
        "v48": [(40.0, 50.0), (0.0, 1.0), (0.5, 47.99)],              # the last one covers almost everything written before
        "nosteps": [(0.0, 1.0)],
        "onestep": [(5.0, 4.0), (28.0, 30.0)]}                        # an inverted span
EXTRA_ASR_ROWS = {"v30": 2}


def step(i, heading, s, e):
    return {"index": i, "heading": heading, "absolute_bounds": [s, e]}


def ann(name, bounds, steps, relevant=True, clip=True):
    return {"relevant": relevant, "clip": clip, "v_duration": VIDEOS[name][1] if name in VIDEOS else 61.0, "bounds": bounds, "steps": steps}


def split():
    return {
        "make a paper plane": {
            "v5.mp4": ann("v5.mp4", [0, 4], [step(0, "fold the sheet", 0, 2), step(1, " crease it ", 2, 4)]),
            "v30.mp4": ann("v30.mp4", [3, 27], [step(0, "fold the wings down", 3, 9), step(1, "same second", 9, 9), step(2, "throw", 12, 27)]),
            "skipA.mp4": ann("skipA.mp4", [], [], relevant=False)},
        "how to tie a bow tie": {
            "v8.mp4": ann("v8.mp4", [1, 7], [step(0, "cross", 1, 3), step(1, "loop", 3, 5), step(2, "pull it tight now please and smile for the camera ok then done", 5, 7)]),
            "skipB.mp4": ann("skipB.mp4", [0, 10], [step(0, "x", 0, 10)], clip=False),
            "v95.mp4": ann("v95.mp4", [10, 90], [step(0, "one", 10, 30), step(1, "two", 30, 32), step(2, "three", 40, 94)])},
        "cook rice in a pot": {
            "v48.mp4": ann("v48.mp4", [0, 47], [step(0, "rinse", 0, 20), step(1, "boil", 20, 47)]),
            "nosteps.mp4": ann("nosteps.mp4", [2, 9], []),
            "onestep.mp4": ann("onestep.mp4", [4, 20], [step(0, "wait", 4, 20)])},
    }


def features(name):
    """Values exact in fp32 that tell video, row and column apart."""
    n = VIDEOS[name][0]
    v = list(VIDEOS).index(name) + 1
    return (v * 1000.0 + torch.arange(n, dtype=torch.float32)[:, None] + torch.arange(D, dtype=torch.float32)[None, :] / 16.0)


def asr_features(vid):
    rows = len(SUBS[vid]) + EXTRA_ASR_ROWS.get(vid, 0)
    v = list(SUBS).index(vid) + 1
    return -(v * 100.0 + torch.arange(rows, dtype=torch.float32)[:, None] + torch.arange(DA, dtype=torch.float32)[None, :] / 8.0)


def stamp(t):
    ms = int(round(t * 1000))
    return f"{ms // 3600000:02d}:{ms // 60000 % 60:02d}:{ms // 1000 % 60:02d},{ms % 1000:03d}"


def srt_text(vid):
    return "".join(f"{i + 1}\n{stamp(s)} --> {stamp(e)}\nsubtitle {i + 1} of {vid}\n\n" for i, (s, e) in enumerate(SUBS[vid]))


def stub_srt_parse(text):
    """All that the reference reads of srt.parse's result: objects with ``start`` / ``end`` timedeltas, in file order."""
    out = []
    for m in re.finditer(r"^(\d\d):(\d\d):(\d\d),(\d\d\d) --> (\d\d):(\d\d):(\d\d),(\d\d\d)$", text, re.M):
        h0, m0, s0, ms0, h1, m1, s1, ms1 = (int(g) for g in m.groups())
        out.append(types.SimpleNamespace(start=datetime.timedelta(hours=h0, minutes=m0, seconds=s0, milliseconds=ms0),
                                         end=datetime.timedelta(hours=h1, minutes=m1, seconds=s1, milliseconds=ms1)))
    return out


def plain(v):
    if torch.is_tensor(v):
        return v.tolist()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def main():
    mg.install_stubs()
    stubs = tempfile.mkdtemp(prefix="hirest_stubs3_")          # what clip4caption/modules/file_utils.py imports and never uses here
    os.makedirs(f"{stubs}/botocore")
    for mod, body in {"boto3": "", "botocore/__init__": "", "botocore/exceptions": "class ClientError(Exception):\n    pass\n"}.items():
        with open(f"{stubs}/{mod}.py", "w") as f:
            f.write(body)
    sys.path.insert(0, stubs)
    sys.path.insert(0, mg.REF)
    sys.path.append(f"{mg.REF}/clip4caption")                # hirest_dataset.py:119 appends it relative to the working directory
    if not hasattr(np, "long"):
        np.long = np.int64                                   # hirest_dataset.py:535 predates numpy 1.24
    import hirest_dataset as ref_ds
    from modules import tokenization
    tokenization.BertTokenizer.from_pretrained = classmethod(lambda cls, *a, **k: _Tok())
    ref_ds.srt.parse = stub_srt_parse
    d = tempfile.mkdtemp(prefix="hirest_loader_")
    assert "train" not in d and "temp" not in d
    for sub in ("feats", "srt", "asr"):
        os.makedirs(f"{d}/{sub}")
    arrays = {}
    for name in VIDEOS:
        torch.save(features(name), f"{d}/feats/{name}.pt")
        arrays[f"feat.{name}"] = features(name).numpy()
    for vid in SUBS:
        with open(f"{d}/srt/{vid}.srt", "w") as f:
            f.write(srt_text(vid))
        torch.save(asr_features(vid), f"{d}/asr/{vid}.pt")
        arrays[f"asr.{vid}"] = asr_features(vid).numpy()
    for name in ("all_data_train.json", "all_data_test.json"):
        json.dump(split(), open(f"{d}/{name}", "w"), indent=2)

    configs = []
    plans = [(task, sp, F, bs, False) for task, sp in (("moment_retrieval", "test"), ("moment_segmentation", "train"),
                                                      ("moment_segmentation", "test"), ("step_captioning", "test"))
             for F in (-1, 8, 48) for bs in (1, 3)]
    plans += [("moment_retrieval", "test", 8, 3, True), ("moment_segmentation", "test", 8, 3, True)]     # end_to_end keeps the video without steps
    for ci, (task, sp, F, bs, e2e) in enumerate(plans):
        args = types.SimpleNamespace(end_to_end=e2e, max_words=MAX_WORDS)
        ds = ref_ds.MomentDataset(args, data_path=Path(d) / f"all_data_{sp}.json", video_dir=None, video_feature_dir=f"{d}/feats",
                                  asr_dir=f"{d}/srt", asr_feature_dir=f"{d}/asr", n_model_frames=F, task=task)
        cfg = {"task": task, "split": sp, "n_model_frames": F, "batch_size": bs, "end_to_end": e2e,
               "examples": [{k: plain(v) for k, v in datum.items()} for datum in ds.data], "batches": []}
        for lo in range(0, len(ds), bs):
            batch = ds.collate_fn([ds[i] for i in range(lo, min(lo + bs, len(ds)))])
            entry = {}
            for k, v in batch.items():
                if torch.is_tensor(v):
                    key = f"c{ci}.b{len(cfg['batches'])}.{k}"
                    arrays[key] = v.numpy()
                    entry[k] = {"npz": key, "dtype": str(v.dtype), "shape": list(v.shape)}
                else:
                    entry[k] = {"value": plain(v)}
            cfg["batches"].append(entry)
        configs.append(cfg)
        print(ci, task, sp, F, bs, e2e, len(ds), "examples", len(cfg["batches"]), "batches", flush=True)

    # the properties the fixture is there for
    by = {(c["task"], c["split"], c["n_model_frames"], c["batch_size"], c["end_to_end"]): c for c in configs}
    r = by[("moment_retrieval", "test", -1, 3, False)]
    assert [e["fname"] for e in r["examples"]] == ["v5.mp4", "v30.mp4", "v8.mp4", "v95.mp4", "v48.mp4", "nosteps.mp4", "onestep.mp4"]
    assert r["batches"][0]["vis_feats"]["shape"] == [3, 30, D] and r["batches"][1]["vis_feats"]["shape"] == [3, 95, D]
    assert all(e["fname"] != "nosteps.mp4" for e in by[("moment_segmentation", "test", 8, 3, False)]["examples"])
    assert any(e["fname"] == "nosteps.mp4" for e in by[("moment_segmentation", "test", 8, 3, True)]["examples"])
    assert all(e["fname"] != "onestep.mp4" for e in by[("moment_segmentation", "train", 8, 3, False)]["examples"])       # two boundaries only
    cap = by[("step_captioning", "test", 8, 1, False)]
    assert any(sum(e["moment_mask"]) == 1 for e in cap["examples"]), "one step starts and ends in the same frame"
    assert any(len([w for w in e["target_text"][6][0] if w]) == MAX_WORDS for e in cap["examples"]), "one caption is cut to max_words"

    class FakeLoader:
        def __init__(self, task, n):
            self.task, self.n = task, n

        def __len__(self):
            return self.n
    multitask = {}
    for sampling in ("roundrobin", "balanced"):
        ml = ref_ds.MultitaskLoader([FakeLoader("moment_retrieval", 3), FakeLoader("moment_segmentation", 5), FakeLoader("step_captioning", 2)],
                                    sampling=sampling, verbose=False)
        multitask[sampling] = []
        for epoch in range(3):
            ml.set_epoch(epoch)
            multitask[sampling].append(list(ml.epoch_tasks))
    # the per-configuration records (every example, every batch) are a few hundred KB of JSON text: kept compressed inside the npz
    arrays["configs.json"] = np.frombuffer(json.dumps(configs).encode(), dtype=np.uint8)
    mg.save("loader_a.npz", **arrays)
    out = {"D": D, "Da": DA, "max_words": MAX_WORDS, "videos": {k: v[0] for k, v in VIDEOS.items()}, "split": split(),
           "srt": {vid: srt_text(vid) for vid in SUBS}, "spans": {vid: [[int(s), int(e)] for s, e in SUBS[vid]] for vid in SUBS},
           "multitask_lengths": [3, 5, 2], "multitask": multitask}
    with open(os.path.join(HERE, "loader_a.json"), "w") as f:
        json.dump(out, f)
    print("loader_a.json", os.path.getsize(os.path.join(HERE, "loader_a.json")) // 1024, "KiB")


if __name__ == "__main__":
    main()
