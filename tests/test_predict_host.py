"""Host side of hirest_amd.predict (no GPU): the rank merge, the per-task dict assembly and the loss average of
``Trainer.predict`` (run.py:607-835), against the reference's rules written out by hand."""
import json
import os

import numpy as np
import pytest

from hirest_amd.predict import mean_loss, merge_rank_results, task_results


def _rank(task, k, n, has_target, scores=False):
    r = {"tasks": [task] * n, "prompts": [f"p{k}{i}" for i in range(n)], "predictions": [[k, i] for i in range(n)],
         "video_fnames": [f"v{k}{i}" for i in range(n)], "video_duration": [10.0 * k + i for i in range(n)]}
    if has_target:
        r["targets"], r["loss"] = [[k, i, "t"] for i in range(n)], [0.5 + k, 1.5 + k]
    if scores:
        r["boundary_scores"] = [[0.1 * k] for _ in range(n)]
    return r


@pytest.mark.parametrize("task", ["moment_retrieval", "moment_segmentation", "step_captioning"])
def test_merge_rank_results_with_targets(task):
    a, b = _rank(task, 1, 2, True, scores=True), _rank(task, 2, 3, True)
    m = merge_rank_results([a, b], task, True)
    for k in ("predictions", "tasks", "video_fnames", "prompts", "video_duration", "targets", "loss"):
        assert m[k] == a[k] + b[k], k                      # rank order, nothing dropped or reordered
    assert m["boundary_scores"] == a["boundary_scores"]   # optional per rank, always present in the result (run.py:661-671)
    assert set(m) == {"predictions", "tasks", "video_fnames", "prompts", "video_duration", "targets", "loss", "boundary_scores"}


def test_merge_rank_results_without_targets():
    # moment segmentation keeps its targets without has_target (run.py:616-617, 679-682); the other tasks carry none
    a, b = _rank("moment_segmentation", 1, 2, False), _rank("moment_segmentation", 2, 1, False)
    a["targets"], b["targets"] = [[1, 5], [2, 6]], [[3, 7]]
    m = merge_rank_results([a, b], "moment_segmentation", False)
    assert m["targets"] == [[1, 5], [2, 6], [3, 7]] and "loss" not in m and m["boundary_scores"] == []
    c = merge_rank_results([_rank("step_captioning", 1, 2, False), _rank("step_captioning", 2, 2, False)], "step_captioning", False)
    assert "targets" not in c and "loss" not in c and len(c["predictions"]) == 4
    # a rank without video names fails as the reference's result['video_fnames'] does
    bad = _rank("step_captioning", 3, 1, False)
    del bad["video_fnames"]
    with pytest.raises(KeyError):
        merge_rank_results([bad], "step_captioning", False)


def test_captioning_dict_with_repeated_videos():
    res = {"tasks": ["step_captioning"] * 4, "prompts": ["p"] * 4, "video_fnames": ["v0", "v1", "v0", "v0"],
           "video_duration": [10.5, 20.0, 11.5, 12.5], "predictions": ["a b", "c", "d e f", ""],
           "targets": ["ta", "tb", "tc", "td"], "loss": [1.0, 2.0]}
    out = task_results(res, True)
    assert list(out) == ["v0", "v1", "loss"]               # first appearance order, the loss last (run.py:832-833)
    assert out["v0"] == {"captions": [{"sentence": "a b"}, {"sentence": "d e f"}, {"sentence": ""}], "video_duration": 12.5,
                         "target_captions": ["ta", "tc", "td"]}          # the duration of the video's LAST sample (run.py:820-821)
    assert out["v1"] == {"captions": [{"sentence": "c"}], "video_duration": 20.0, "target_captions": ["tb"]}
    assert out["loss"] == 1.5
    plain = task_results({k: v for k, v in res.items() if k not in ("targets", "loss")}, False)
    assert "loss" not in plain and "target_captions" not in plain["v0"] and len(plain["v0"]["captions"]) == 3
    with pytest.raises(AssertionError):                    # run.py:689: equal list lengths
        task_results(dict(res, prompts=["p"] * 3), True)
    with pytest.raises(AssertionError):                    # run.py:693
        task_results(dict(res, predictions=["a"] * 3), True)


def test_mean_of_fp32_rounded_losses():
    vals = np.array([0.1, 10.394904, 1.0751274, 3.3333333], dtype=np.float32)
    as_items = [float(v) for v in vals]                    # loss.item(): the fp32 value widened to double
    want = np.mean(as_items)
    assert mean_loss(as_items) == want and isinstance(mean_loss(as_items), np.floating)
    assert mean_loss(as_items) != np.mean([0.1, 10.394904, 1.0751274, 3.3333333])      # not the mean of the unrounded numbers
    assert mean_loss(as_items) != float(vals.mean())                                    # nor a float32 accumulation


def test_segmentation_short_bounds_and_retrieval_on_host():
    # one bin per second (n_model_frames = -1): an index at or past int(duration) raises in the reference; the pair stays short
    res = {"tasks": ["moment_segmentation"] * 2, "prompts": ["p", "q"], "video_fnames": ["v", "w"], "video_duration": [30.5, 8.0],
           "predictions": [[3, 9, 20], [2, 7, 12, 15]], "targets": [[3, 10, 20], [2, 15]]}
    out = task_results(res, False, -1, on_device=False)
    assert out["v"] == {"bounds": [[3, 9], [9, 20]], "video_duration": 30.5, "pred_bounds": [3, 9, 20], "target_bounds": [3, 10, 20]}
    assert out["w"]["bounds"] == [[2, 7], [7], []] and "loss" not in out
    mr = {"tasks": ["moment_retrieval"] * 3, "prompts": ["p", "p", "q"], "video_fnames": ["v", "w", "v"], "video_duration": [30.5, 8.0, 30.5],
          "predictions": [[3, 9], [2, 7], [0, 29]], "targets": [[1, 2], [3, 4], [5, 6]], "loss": [2.0]}
    got = task_results(mr, True, -1, on_device=False)
    assert got == {"p": {"v": {"bounds": [3, 9], "video_duration": 30.5, "target_bounds": [1, 2]},
                         "w": {"bounds": [2, 7], "video_duration": 8.0, "target_bounds": [3, 4]}},
                   "q": {"v": {"bounds": [0, 29], "video_duration": 30.5, "target_bounds": [5, 6]}}, "loss": 2.0}
    with pytest.raises(ValueError):
        task_results(dict(mr, tasks=["other"] * 3), True, -1, on_device=False)


def test_host_assembly_reproduces_the_reference_dicts(golden_dir):
    """The recorded dicts of the reference's own post-processing (tests/golden/valid_predict.json) rebuilt from their own lists:
    timestamps, short bounds, key order."""
    from hirest_amd.synth import TRAIN_CASES, valid_batches
    ref = json.load(open(os.path.join(golden_dir, "valid_predict.json")))["moment_segmentation.plain.beam5"]
    batches = [valid_batches(c)["moment_segmentation"] for c in TRAIN_CASES]
    res = {k: [x for b in batches for x in b[k]] for k in ("tasks", "prompts", "video_fnames", "video_duration")}
    res["predictions"] = [ref[v]["pred_bounds"] for v in res["video_fnames"]]
    res["targets"] = [x for b in batches for x in b["all_bound_frames"]]
    out = task_results(res, False, -1, on_device=False)
    assert out == ref and list(out) == list(ref)
    assert any(len(b) < 2 for v in out.values() for b in v["bounds"])     # the fixture does hold short pairs
