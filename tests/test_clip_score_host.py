"""CLIPScore (evaluate.py:190-320) on the host: the selection of frames, skips, candidates and categories against the real
reference's recorded run (tests/golden/clipscore.json, written by make_clipscore_golden.py), the error rules, and the
hirest_clip_score C entry point's argument checks (no device needed)."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from hirest_amd import evaluation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "clipscore.json")) as f:
        return json.load(f)


def write_frames(root):
    """The fixture's JPEG bytes as <root>/<video>/<frame>.jpg; returns the frame directory."""
    g = np.load(os.path.join(GOLDEN, "clipscore.npz"))
    with open(os.path.join(GOLDEN, "clipscore.json")) as f:
        names = json.load(f)["files"]
    blob, offs = g["jpeg_blob"], g["jpeg_offsets"]
    frame_dir = os.path.join(str(root), "frames")
    for i, rel in enumerate(names):
        path = os.path.join(frame_dir, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(blob[offs[i]:offs[i + 1]].tobytes())
    return frame_dir


@pytest.fixture(scope="module")
def frame_dir(tmp_path_factory):
    return write_frames(tmp_path_factory.mktemp("clipscore"))


def _calls(plan, frame_dir):
    return [{"candidate": plan.candidates[k], "frames": [os.path.relpath(plan.frames[r], frame_dir) for r in plan.sel[j]]}
            for j, k in enumerate(plan.scored)]


def test_selection_matches_reference_without_categories(golden, frame_dir):
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir, golden["video_to_cat"], per_category=False)
    want = [{"candidate": c["candidate"], "frames": c["frames"]} for c in golden["runs"]["all"]["calls"]]
    assert _calls(plan, frame_dir) == want
    assert list(plan.categories) == ["all"]
    assert plan.categories["all"]["Total"] == golden["runs"]["all"]["result"]["all"]["Total"]
    assert plan.tokens.shape == (len(want), 77)
    # every unique file once, and every file the reference opened is among them
    assert len(set(plan.frames)) == len(plan.frames)
    assert {f for c in want for f in c["frames"]} == {os.path.relpath(f, frame_dir) for f in plan.frames}
    assert sum(plan.skip) == len(plan.captions) - len(want)


def test_selection_matches_reference_per_category(golden, frame_dir):
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir, golden["video_to_cat"], per_category=True)
    ref = golden["runs"]["per_category"]
    assert set(plan.categories) == set(ref["result"])
    for c, m in plan.categories.items():
        assert m["Total"] == ref["result"][c]["Total"], c
    # the reference re-runs CLIP per category, in its category order (here sorted + "all"): the concatenation of each category's
    # scored captions
    pos = {k: j for j, k in enumerate(plan.scored)}
    calls = _calls(plan, frame_dir)
    seq = [calls[pos[k]] for c in sorted(plan.categories, key=lambda c: (c == "all", c)) for k in plan.categories[c]["captions"]
           if k in pos]
    assert seq == [{"candidate": c["candidate"], "frames": c["frames"]} for c in ref["calls"]]
    # the empty categories: one whose only GT video has no captions, one with no GT video at all
    assert "Pets and Animals" not in plan.categories and "Sports and Fitness" not in plan.categories
    assert "Health" in plan.categories                       # its video has captions, all skipped (no frame directory)


def test_integer_frame_sort_and_negative_index(golden, frame_dir):
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir)
    rel = [os.path.relpath(f, frame_dir) for f in plan.frames]
    sel = {plan.captions[k]: [rel[r] for r in plan.sel[j]] for j, k in enumerate(plan.scored)}
    # unpadded.mp4 frames 1..12: index 8 -> frame_9, index 9 -> frame_10 (a lexical sort would put frame_10 after frame_1)
    assert sel[("unpadded.mp4", 2)] == ["unpadded.mp4/frame_10.jpg"] * 4        # linspace(9, 9, 4)
    assert sel[("unpadded.mp4", 0)] == ["unpadded.mp4/frame_8.jpg", "unpadded.mp4/frame_8.jpg", "unpadded.mp4/frame_9.jpg",
                                        "unpadded.mp4/frame_10.jpg"]                     # linspace(7, 9, 4) = 7, 7.67, 8.33, 9
    # start == end == 0: linspace(0, -1, 4).astype(int) = [0, 0, 0, -1] -> the last frame
    assert sel[("nWBuM3LNTcM.mp4", 3)][-1] == "nWBuM3LNTcM.mp4/frame_000039.jpg"
    assert all(plan.skip[plan.captions.index(("nodir.mp4", i))] for i in range(2))


def test_candidate_is_the_prediction_lowercased(golden, frame_dir):
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir)
    for (v, i), cand in zip(plan.captions, plan.candidates):
        assert cand == golden["pred"][v]["captions"][i]["sentence"].lower()


def test_no_frame_dir_scores_zero(golden):
    for fd in (None, "None"):
        plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], fd, golden["video_to_cat"], per_category=True)
        assert plan.scored == [] and all(plan.skip) and plan.frames == []
        # no model and no device is touched when nothing is scored
        res = evaluation.evaluate_clip_score(golden["gt"], golden["pred"], golden["video_to_cat"], None, fd, per_category=True)
        assert res == golden["result_no_frames"]
        assert all(r["CLIPScore"] == 0 for r in res.values())
        assert [s for _, _, s in evaluation.caption_clip_scores(golden["gt"], golden["pred"], None, fd)] == [None] * len(plan.captions)


def test_long_candidate_raises(golden, frame_dir):
    pred = copy.deepcopy(golden["pred"])
    pred["grey.mp4"]["captions"][0]["sentence"] = " ".join(["word"] * 100)
    with pytest.raises(RuntimeError, match="too long"):
        evaluation.clip_score_plan(golden["gt"], pred, frame_dir, golden["video_to_cat"])
    # a skipped caption is never tokenized (evaluate.py:239-243)
    pred = copy.deepcopy(golden["pred"])
    pred["nodir.mp4"]["captions"][0]["sentence"] = " ".join(["word"] * 100)
    evaluation.clip_score_plan(golden["gt"], pred, frame_dir, golden["video_to_cat"])


def test_missing_category_raises(golden, frame_dir):
    cats = dict(golden["video_to_cat"])
    del cats["nocaps.mp4"]                     # even a video without captions is looked up (evaluate.py:219)
    for per_category in (False, True):
        with pytest.raises(KeyError):
            evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir, cats, per_category=per_category)


def test_videos_subset_keeps_reference_order(golden, frame_dir):
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir, videos=["grey.mp4", "nWBuM3LNTcM.mp4"])
    assert [v for v, _ in plan.captions] == ["nWBuM3LNTcM.mp4"] * 8 + ["grey.mp4"] * 3
    with pytest.raises(KeyError):
        evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir, videos=["absent.mp4"])


def test_transformers_features_match_the_oracle_pip_head():
    """transformers' CLIPModel (an independent implementation of the pip `clip` CLS head) against the oracle's restatement, on
    the same tiny weights: what the GPU test then pins the device tower to."""
    from hirest_amd import synth
    from oracle import ref_cpu
    with open(os.path.join(GOLDEN, "clipscore.json")) as f:
        meta = json.load(f)
    g = np.load(os.path.join(GOLDEN, "clipscore.npz"))
    c = synth.OPENAI_VIT_TINY
    sd = synth.openai_clip_state_dict(c, meta["seed"])
    img = synth.frames(meta["hf_image_frames"], (4, 3, 224, 224), meta["hf_image_seed"])
    got_i = ref_cpu.openai_encode_image(sd, img, c, pip_head=True)
    got_t = ref_cpu.openai_encode_text(sd, torch.from_numpy(g["hf_tokens"]), c)
    for got, ref in ((got_i, g["hf_image_features"]), (got_t, g["hf_text_features"])):
        ref = torch.from_numpy(ref)
        assert torch.nn.functional.cosine_similarity(got, ref).min().item() > 1 - 1e-6
        assert ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item() < 1e-5


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_clip_score_argument_errors_without_gpu(lib):
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is rejected before anything is enqueued
    ok = dict(img=p, idt=0, U=8, txt=p, tdt=0, sel=p, C=3, K=4, E=64, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.hirest_clip_score(a["img"], a["idt"], a["U"], a["txt"], a["tdt"], a["sel"], a["C"], a["K"], a["E"], a["out"], None)
    for bad in (dict(img=None), dict(txt=None), dict(sel=None), dict(out=None), dict(idt=2), dict(tdt=2), dict(idt=-1), dict(tdt=7),
                dict(C=-1), dict(K=0), dict(K=-4), dict(E=0), dict(U=0), dict(U=-1)):
        assert call(**bad) == -1, bad
    assert call(C=0) == 0                 # nothing to score: success, nothing launched


def test_clip_score_declared_and_exported(lib):
    from hirest_amd import _lib
    hdr = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    assert "int hirest_clip_score(const void* img_rows, int32_t img_dtype, int32_t U," in hdr
    assert "hirest_clip_score" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hirest_clip_score")
    assert lib.hirest_abi_version() == 4
