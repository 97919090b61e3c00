"""The validation / test pass of the reference's trainer, ``Trainer.predict`` (run.py:521-838), on the device steps of this package.

``predict(model, loader, has_target, ...)`` walks a loader of one task, collects what the reference collects per batch and returns
the per-task dict that ``run.py`` dumps and ``evaluate.py`` reads (run.py:704-835), with ``'loss'`` beside it when the batches
carry targets.  With targets every batch goes through ``MomentModel.valid_step`` (loss and prediction from one forward); without
them through ``test_step``.  Step captioning is captioned by ``caption_batches``, one beam search over several loader batches, with
or without targets; with them each batch's loss comes from its own ``valid_step(batch, search=False)`` first.  The
per-batch losses stay on the device and are read once, after the last batch.

The reference's quirks that show in the output are kept: the ``assert`` on equal list lengths, segmentation ``bounds`` entries left
short where a timestamp conversion raises (run.py:766-774), ``'loss'`` absent without targets, segmentation targets kept without
them."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import timeline

_MERGED = ("predictions", "tasks", "video_fnames", "prompts", "video_duration")


def merge_rank_results(per_rank: Sequence[Dict], task: str, has_target: bool) -> Dict:
    """The concatenation of every rank's lists in rank order with the reference's key handling (run.py:638-682): ``predictions``,
    ``tasks``, ``video_fnames``, ``prompts`` and ``video_duration`` are required of every rank (a missing one raises KeyError there
    too), ``boundary_scores`` is optional per rank and always present in the result, ``loss`` and ``targets`` are merged with
    targets, ``targets`` alone for moment segmentation without them.  Pure host code."""
    out: Dict = {k: [] for k in _MERGED}
    out["boundary_scores"] = []
    for r in per_rank:
        for k in _MERGED:
            out[k].extend(r[k])
        if "boundary_scores" in r:
            out["boundary_scores"].extend(r["boundary_scores"])
    if has_target:
        out["loss"], out["targets"] = [], []
        for r in per_rank:
            out["loss"].extend(r["loss"])
            out["targets"].extend(r["targets"])
    elif task == "moment_segmentation":
        out["targets"] = []
        for r in per_rank:
            out["targets"].extend(r["targets"])
    return out


def mean_loss(losses: Sequence[float]):
    """``np.mean`` of the per-batch losses as Python floats — each the fp32 value of ``loss.item()`` widened to double — which is the
    reference's arithmetic (run.py:562, 695)."""
    return np.mean([float(x) for x in losses])


def task_results(results: Dict, has_target: bool, n_model_frames: int = -1, on_device: bool = True) -> Dict:
    """run.py:689-835: the collected lists -> the dict of the lists' task.  ``on_device``: the timestamps of moment retrieval and
    segmentation through the batched kernels of hirest_amd.timeline; False: through its scalar host function, entry by entry as the
    reference does (same numbers; needs no GPU)."""
    n = len(results["tasks"])
    assert n == len(results["video_fnames"]) == len(results["prompts"]), \
        f"len(tasks)={n}, len(video_fnames)={len(results['video_fnames'])}, len(prompts)={len(results['prompts'])}"
    if has_target:
        assert len(results["predictions"]) == len(results["video_fnames"])
    task = results["tasks"][0]
    videos, durations, preds = results["video_fnames"], results["video_duration"], results["predictions"]
    targets = results.get("targets")
    if task == "moment_retrieval":
        if on_device:
            out = timeline.moment_retrieval_results(preds, results["prompts"], videos, durations, n_model_frames,
                                                    targets if has_target else None)
        else:
            out = {}
            for i in range(len(videos)):
                entry = out.setdefault(results["prompts"][i], {}).setdefault(videos[i], {})
                assert len(preds[i]) == 2
                entry["bounds"] = [timeline.frame_index_to_timestamp(p, durations[i], n_frames=n_model_frames) for p in preds[i]]
                entry["video_duration"] = durations[i]
                if has_target:
                    entry["target_bounds"] = targets[i]
    elif task == "moment_segmentation":
        if on_device:
            out = timeline.moment_segmentation_results(preds, videos, durations, n_model_frames, targets)
        else:
            out = {}
            for i in range(n):
                entry = out.setdefault(videos[i], {})
                bounds = []
                for j in range(len(preds[i]) - 1):
                    bound: List[int] = []
                    try:
                        bound.append(timeline.frame_index_to_timestamp(preds[i][j], durations[i], n_frames=n_model_frames))
                        bound.append(timeline.frame_index_to_timestamp(preds[i][j + 1], durations[i], n_frames=n_model_frames))
                    except Exception:                                     # run.py:771: the pair stays short
                        pass
                    bounds.append(bound)
                entry["bounds"] = bounds
                entry["video_duration"] = durations[i]
                entry["pred_bounds"] = preds[i]
                entry["target_bounds"] = targets[i]
    elif task == "step_captioning":
        out = {}
        for i in range(n):
            entry = out.setdefault(videos[i], {})
            entry.setdefault("captions", []).append({"sentence": preds[i]})
            entry["video_duration"] = durations[i]
            if has_target:
                entry.setdefault("target_captions", []).append(targets[i])
    else:
        raise ValueError("Unknown task: {}".format(task))
    if has_target:
        out["loss"] = mean_loss(results["loss"])
    return out


def _batch_targets(batch, task):
    if task == "moment_retrieval":                                        # run.py:575-580
        return torch.cat([torch.as_tensor(batch["moment_retrieval_start_target"]).view(-1, 1),
                          torch.as_tensor(batch["moment_retrieval_end_target"]).view(-1, 1)], dim=1).cpu().tolist()
    if task == "moment_segmentation":
        return batch["all_bound_frames"]
    return batch["target_text_raw"] if "target_text_raw" in batch else batch["target_text"]


@torch.no_grad()
def predict(model, loader, has_target: bool = False, num_beams: int = 5, n_model_frames: int = -1, group=None) -> Dict:
    """``Trainer.predict(loader, has_target)`` (run.py:521-838) for ``loader.task``; ``num_beams`` and ``n_model_frames`` are the
    reference's ``args.num_beams`` / ``args.n_model_frames``.  ``group``: a torch.distributed process group — every rank's lists are
    gathered and merged in rank order (merge_rank_results), so every rank returns the dict of the whole split."""
    task = loader.task
    batches = list(loader)
    lists: Dict[str, list] = {k: [] for k in ("predictions", "targets", "tasks", "prompts", "video_fnames", "video_duration",
                                              "boundary_scores")}
    losses = []
    if task == "step_captioning":          # one beam search over the union of batches (same captions); with targets, each batch's own loss first
        if has_target:
            losses = [model.valid_step(b, search=False)["loss"].detach().reshape(1).float() for b in batches]
        outs = model.caption_batches(batches, num_beams=num_beams, merge=True)
    else:
        step = model.valid_step if has_target else model.test_step
        outs = []
        for batch in batches:
            res = step(batch, num_beams=num_beams)
            if has_target:
                losses.append(res["loss"].detach().reshape(1).float())    # stays on the device until the end of the pass
            outs.append(res)
    for batch, res in zip(batches, outs):
        lists["predictions"].extend(res["prediction"])
        lists["targets"].extend(_batch_targets(batch, task) if has_target or task == "moment_segmentation" else [])
        lists["tasks"].extend(batch["tasks"])
        lists["prompts"].extend(batch["prompts"])
        for k in ("video_fnames", "video_duration"):
            if k in batch:
                lists[k].extend(batch[k])
        if "boundary_scores" in res:
            lists["boundary_scores"].extend(res["boundary_scores"])
    results: Dict = {"tasks": lists["tasks"], "prompts": lists["prompts"], "predictions": lists["predictions"]}
    if has_target:
        results["targets"] = lists["targets"]
        results["loss"] = torch.cat(losses).cpu().tolist() if losses else []          # the one read of the losses
    elif task == "moment_segmentation":
        results["targets"] = lists["targets"]
    for k in ("boundary_scores", "video_fnames", "video_duration"):
        if lists[k]:
            results[k] = lists[k]
    if group is not None:
        import torch.distributed as dist
        gathered: List[Optional[Dict]] = [None] * dist.get_world_size(group)
        dist.all_gather_object(gathered, results, group=group)
        results = merge_rank_results(gathered, task, has_target)
    return task_results(results, has_target, n_model_frames)
