#!/usr/bin/env python3
"""Generate tests/golden/cascade_a.{npz,json}: the REAL reference's end-to-end chain (run.py:383-490) on a small synthetic split.

Runs only where the reference checkout is available (see make_golden.py, whose stubs and model construction it reuses).  The
pieces that run are the reference's own: ``MomentModel.test_step`` for all three tasks, ``frame_index_to_timestamp``, and the
``MomentDataset`` constructor / ``__getitem__`` / ``collate_fn`` with ``args.end_to_end = True`` reading the rewritten
``all_data_test.json`` from a throw-away data directory.  What run.py does inline in ``Trainer.test`` / ``Trainer.predict`` —
collecting predictions into result dicts and rewriting the JSON between the stages — is restated here line by line with its
run.py line numbers, on the data the reference's functions returned.

Weights come from ``hirest_amd.synth`` by seed (as for every joint_* fixture; [SEP] is biased up as for the caption_* fixtures)
and are not stored.  The inputs are stored: frame / ASR / text features rounded to bf16-representable values (kept as their
uint16 bit patterns, so the file stays small and the values exact), durations and the split.  Stored results: every
intermediate integer of the chain, the token ids at beam 3 and beam 5, and the final dict at either beam width.

    python tests/golden/make_cascade_golden.py
"""
import copy
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository on sys.path)
from hirest_amd import synth  # noqa: E402

B, T = 3, 48                      # three processed videos, 48 model frames each (args.n_model_frames = 48)
V_DURATION = [47.6, 30.2, 95.4]   # rounds to 48 / 30 / 95 seconds: two samples whose bins are not one per second
FIRST_SEED, N_SEEDS = 1, 400
PROMPTS = ["make a paper plane", "how to tie a bow tie", "cook rice in a pot"]
VIDEOS = ["vidA.mp4", "vidB.mp4", "vidC.mp4"]


def to_bf16_exact(t):
    return t.to(torch.bfloat16).float()


def bf16_bits(t):
    return (t.contiguous().view(torch.int32).numpy().astype(np.uint32) >> 16).astype(np.uint16)


def inputs(seed):
    vis = synth.tensor("cascade.a.vis", (B, T, 1024), 1.0, seed)
    vis = to_bf16_exact(vis / vis.norm(dim=-1, keepdim=True))
    asr = synth.tensor("cascade.a.asr", (B, T, 384), 0.05, seed)
    gaps = synth.uniform_pm1("cascade.a.gap", B * T, seed).reshape(B, T) > 0.2
    asr = to_bf16_exact(asr * torch.from_numpy(~gaps).float()[..., None])
    text = to_bf16_exact(synth.tensor("cascade.a.text", (B, 1024), 1.0, seed))
    return vis, asr, text


def split():
    """A HiREST-style split: per prompt one processed video and videos the loader skips (hirest_dataset.py:131-134)."""
    data = {}
    for i, (p, v) in enumerate(zip(PROMPTS, VIDEOS)):
        data[p] = {v: {"relevant": True, "clip": True, "v_duration": V_DURATION[i], "bounds": [3, 20 + i],
                       "steps": [{"index": 0, "heading": "first", "absolute_bounds": [3, 9]},
                                 {"index": 1, "heading": "second", "absolute_bounds": [9, 20 + i]}]},
                   f"skip{i}.mp4": {"relevant": False, "clip": False, "v_duration": 61.0 + i, "bounds": [], "steps": []}}
    data[PROMPTS[0]]["whole.mp4"] = {"relevant": True, "clip": False, "v_duration": 12.3, "bounds": [0, 12], "steps": []}
    return data


class _Tok:
    """The BertTokenizer stub: ids <-> decimal strings (no vocabulary file offline)."""
    vocab = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102}

    def tokenize(self, text):
        return text.split()

    def convert_tokens_to_ids(self, toks):
        return [self.vocab.get(t, 100) for t in toks]

    def convert_ids_to_tokens(self, ids):
        return [str(i) for i in ids]


def main():
    mg.install_stubs()
    model, args = mg.build_reference_moment_model()
    if not hasattr(np, "long"):
        np.long = np.int64                                   # hirest_dataset.py:535 predates numpy 1.24
    import hirest_dataset as ref_ds
    from modules import tokenization
    tokenization.BertTokenizer.from_pretrained = classmethod(lambda cls, *a, **k: _Tok())
    names = [k for k in model.state_dict().keys() if not k.startswith("clip_model.")]
    shapes = {k: tuple(model.state_dict()[k].shape) for k in names}
    sd = synth.joint_state_dict(shapes, 31)
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5
    print(model.load_state_dict(sd, strict=False))
    args.end_to_end = True
    args.n_model_frames = T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    durations = [round(d) for d in V_DURATION]

    def dataset(data_dir, task):
        """The real MomentDataset (its own constructor), as get_moment_loader builds it (hirest_dataset.py:591-600) without ASR
        directories; the ASR features are attached to the collated batch below."""
        return ref_ds.MomentDataset(args, data_path=Path(data_dir) / "all_data_test.json", video_dir=None,
                                    video_feature_dir=str(Path(data_dir) / "feats"), asr_dir=None, asr_feature_dir=None,
                                    n_model_frames=args.n_model_frames, task=task)

    def batch_of(ds, asr, text_of):
        batch = ds.collate_fn([ds[i] for i in range(len(ds))])
        batch["asr_feats"] = torch.stack([asr[VIDEOS.index(f)] for f in batch["video_fnames"]])
        model.clip_model.encode_text = lambda ids, _p=batch["prompts"]: torch.stack([text_of[p] for p in _p])
        return batch

    def chain(seed, beams_list):
        vis, asr, text = inputs(seed)
        text_of = {p: text[i] for i, p in enumerate(PROMPTS)}
        d = tempfile.mkdtemp(prefix="hirest_cascade_")
        assert "train" not in d and "temp" not in os.path.basename(d)
        os.makedirs(f"{d}/feats")
        for i, v in enumerate(VIDEOS):
            torch.save(vis[i].clone(), f"{d}/feats/{v}.pt")
        test0 = split()
        path = f"{d}/all_data_test.json"
        json.dump(test0, open(path, "w"), indent=2)
        out = {"seed": seed}
        with torch.no_grad():
            # ---- stage 1: moment retrieval (run.py:389, predict :546-746)
            ds = dataset(d, "moment_retrieval")
            batch = batch_of(ds, asr, text_of)
            assert batch["video_fnames"] == VIDEOS and batch["prompts"] == PROMPTS and batch["video_duration"] == durations
            assert torch.equal(batch["vis_feats"], vis) and bool(batch["moment_mask"].all()) and bool(batch["vis_mask"].all())
            pred = model.test_step(batch)["prediction"]
            moments = {}
            for i in range(B):                                                             # run.py:719-737
                s = ref_ds.frame_index_to_timestamp(pred[i][0], batch["video_duration"][i], n_frames=args.n_model_frames)
                e = ref_ds.frame_index_to_timestamp(pred[i][1], batch["video_duration"][i], n_frames=args.n_model_frames)
                moments.setdefault(batch["prompts"][i], {})[batch["video_fnames"][i]] = {"bounds": [s, e]}
            test = json.load(open(path))
            for prompt in test:                                                            # run.py:401-416
                if prompt not in moments:
                    continue
                for video in test[prompt]:
                    if video not in moments[prompt]:
                        continue
                    test[prompt][video]["bounds"] = moments[prompt][video]["bounds"]
                    test[prompt][video]["steps"] = [{"index": i, "heading": "", "absolute_bounds": [i, i + 1]} for i in range(5)]
            json.dump(test, open(path, "w"), indent=2)
            out["moment_frames"] = [[int(x) for x in p] for p in pred]
            out["bounds"] = [moments[p][v]["bounds"] for p, v in zip(PROMPTS, VIDEOS)]
            # ---- stage 2: moment segmentation (run.py:422-456, predict :758-782)
            ds = dataset(d, "moment_segmentation")
            batch = batch_of(ds, asr, text_of)
            assert batch["video_fnames"] == VIDEOS
            out["bound_frames"] = batch["moment_bound_frames"].tolist()
            seg = model.test_step(batch)["prediction"]
            out["boundary_frames"] = [[int(x) for x in p] for p in seg]
            if any(len(p) < 2 for p in seg):
                return out, None                              # the reference raises in the captioning dataset (hirest_dataset.py:279)
            moments = {}
            for i in range(B):                                                             # run.py:758-776
                bounds = []
                for j in range(len(seg[i]) - 1):
                    bounds.append([ref_ds.frame_index_to_timestamp(seg[i][j], batch["video_duration"][i], n_frames=args.n_model_frames),
                                   ref_ds.frame_index_to_timestamp(seg[i][j + 1], batch["video_duration"][i], n_frames=args.n_model_frames)])
                moments[batch["video_fnames"][i]] = {"bounds": bounds}
            test = json.load(open(path))
            for prompt in test:                                                            # run.py:441-453
                for video in test[prompt]:
                    test[prompt][video]["steps"] = []
                    if video not in moments:
                        continue
                    for i, bound in enumerate(moments[video]["bounds"]):
                        test[prompt][video]["steps"].append({"index": i, "heading": "", "absolute_bounds": bound})
            json.dump(test, open(path, "w"), indent=2)
            out["step_bounds"] = [moments[v]["bounds"] for v in VIDEOS]
            # ---- stage 3: step captioning (run.py:459-485, predict :803-817)
            ds = dataset(d, "step_captioning")
            batch = batch_of(ds, asr, text_of)
            sel = [torch.nonzero(m).flatten().tolist() for m in batch["moment_mask"]]
            out["step_sample"] = [VIDEOS.index(f) for f in batch["video_fnames"]]
            out["step_mask_frames"] = sel                     # the frames each step's captioning mask selects
            out["step_frames"] = [[ref_ds.timestamp_to_frame_index(t, durations[b], n_frames=args.n_model_frames) for t in pair]
                                  for b in range(B) for pair in out["step_bounds"][b]]     # hirest_dataset.py:289-290
            out["trimmed_rows"] = None
            props = {"min_steps": min(len(s) for s in out["step_bounds"]), "max_steps": max(len(s) for s in out["step_bounds"]),
                     "longest_moment": max(f[1] - f[0] + 1 for f in out["bound_frames"]),
                     "shortest_step": min(len(s) for s in sel), "longest_step": max(len(s) for s in sel)}
            out["properties"] = props
            if beams_list is None:
                return out, props
            trimmed = model.trim_feats(batch["vis_feats"], batch["moment_mask"], len(sel), batch["vis_feats"].device)
            out["trimmed_rows"] = mg.np32(trimmed[:, [0, 7, 19]])
            out["token_ids"], out["final"] = {}, {}
            for beams in beams_list:
                cap = model.test_step(batch, num_beams=beams)["prediction"]
                captions = {}
                for i, f in enumerate(batch["video_fnames"]):                              # run.py:803-817
                    captions.setdefault(f, {"captions": []})["captions"].append({"sentence": cap[i]})
                final = json.load(open(path))
                for prompt in final:                                                       # run.py:476-480
                    for video in final[prompt]:
                        if video in captions:
                            for i, sent in enumerate(captions[video]["captions"]):
                                final[prompt][video]["steps"][i]["heading"] = sent["sentence"]
                out["token_ids"][str(beams)] = [[int(x) for x in c.split()] for c in cap]
                out["final"][str(beams)] = final
        return out, props

    found = None
    for seed in range(FIRST_SEED, FIRST_SEED + N_SEEDS):
        out, props = chain(seed, None)
        print(seed, out["moment_frames"], out["boundary_frames"], props, flush=True)
        if props is None:
            continue
        requant = any(out["bound_frames"][b] != out["moment_frames"][b] for b in range(B))
        if (props["min_steps"] >= 1 and props["max_steps"] >= 3 and props["longest_moment"] > 20 and props["shortest_step"] < 20
                and requant):
            found = seed
            break
    assert found is not None, "no seed gives the required properties"
    out, props = chain(found, [3, 5])
    # the properties the fixture is chosen for
    assert props["min_steps"] >= 1, "every sample has at least one step (else the reference raises)"
    assert props["max_steps"] >= 3, "one sample has three or more steps"
    assert props["longest_moment"] > 20, "one retrieved moment is longer than 20 frames (truncation)"
    assert props["shortest_step"] < 20, "one step is shorter than 20 frames (repetition)"
    assert any(durations[b] != T for b in range(B)) and any(out["bound_frames"][b] != out["moment_frames"][b] for b in range(B)), \
        "the frame -> second -> frame re-quantisation is not the identity for one sample"
    vis, asr, text = inputs(found)
    trimmed = out.pop("trimmed_rows")
    mg.save("cascade_a.npz", vis_bf16=bf16_bits(vis), asr_bf16=bf16_bits(asr), text_bf16=bf16_bits(text),
            durations=np.array(durations, dtype=np.int64), trimmed_rows=trimmed)
    out.update({"B": B, "T": T, "n_model_frames": T, "prompts": PROMPTS, "video_fnames": VIDEOS, "durations": durations,
                "split": split()})
    with open(os.path.join(HERE, "cascade_a.json"), "w") as f:
        json.dump(out, f)
    print(json.dumps({k: v for k, v in out.items() if k not in ("final", "split")}))


if __name__ == "__main__":
    main()
