"""Moment-task metrics of the reference's evaluate.py with the interval arithmetic on the GPU, same function
names and dict layouts, so a driver holding predictions can score them without the JSON round trip the reference makes
(``run.py`` dumps predictions, ``evaluate.py`` re-reads them):

    evaluate_video_retrieval(gt, pred, prompt_to_cat)       # evaluate.py:33-81    R@1/5/10/50 with the (score, name) tie rule
    evaluate_moment_retrieval(gt, pred, prompt_to_cat)      # evaluate.py:83-121   R@0.5 / R@0.7 per prompt category
    compute_step_bound_scores(gt, pred, video_to_cat)       # evaluate.py:123-188  step recall / precision at tIoU
    preprocess_moment_bounds(gt, pred)                      # evaluate.py:322-412  filter + NMS + gap filling
    evaluate_clip_score(gt, pred, video_to_cat, model, dir) # evaluate.py:190-320  the CLIPScore leg of step captioning
    evaluate_bert_score(gt, pred, video_to_cat, scorer)     # evaluate.py:190-320  the BERTScore_F1 leg of step captioning

``gt`` / ``pred`` are the reference's dicts (or JSON paths).  The category maps are arguments (the reference reads them
into module globals in ``__main__``, :444-466).  Intervals are flattened to float64 tensors, the per-pair / per-video
work runs in ``csrc/eval.hip`` in double precision with Python's operation order (identical decisions), and the final
means are taken on the host in the reference's summation order, so results are equal to the last bit.
Tensor-level entry points (`interval_iou`, `step_bound_pr`, `preprocess_bounds`) take device tensors directly.
No CPU fallback.  CLIPScore runs as a batch: frames decoded and encoded once on the device, one scoring kernel
(``csrc/score.hip``); BERTScore likewise: unique sentences encoded once, one matching kernel (``csrc/bertscore.hip``).  The other
caption metrics (entailment / COCO, :190-320) are out of scope.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops


def _load(x):
    if isinstance(x, str):
        with open(x, "r") as f:
            return json.load(f)
    assert isinstance(x, dict), "data should be a str path or a dict"          # evaluate.py:7-22
    return x


def _dev(device):
    device = torch.device(device if device is not None else "cuda:0")
    if device.type != "cuda":
        raise RuntimeError("hirest_amd.evaluation runs on MI355X only (no CPU fallback)")
    return device


def _categories(cat_map: Dict[str, str]) -> List[str]:
    return sorted(set(cat_map.values())) + ["all"]


# ------------------------------------------------------------------------------------------------ tensor level

def interval_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """compute_iou(a[i], b[i]) for [n,2] float64 CUDA tensors."""
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape and a.shape[-1] == 2 and a.is_cuda
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    _lib.check(_lib.load().hirest_interval_iou_f64(a.data_ptr(), b.data_ptr(), a.shape[0], out.data_ptr(), ops.stream_ptr()),
               "hirest_interval_iou_f64")
    return out


def step_bound_pr(refs: torch.Tensor, ref_off: torch.Tensor, preds: torch.Tensor, pred_off: torch.Tensor, tiou: float):
    """Ragged per-video step recall / precision; returns (recall[V], precision[V], best_iou[sum preds])."""
    V = ref_off.numel() - 1
    dev = refs.device
    rec = torch.empty(V, dtype=torch.float64, device=dev)
    prc = torch.empty(V, dtype=torch.float64, device=dev)
    best = torch.empty(preds.shape[0], dtype=torch.float64, device=dev)
    _lib.check(_lib.load().hirest_step_bound_pr(refs.data_ptr(), ref_off.data_ptr(), preds.data_ptr(), pred_off.data_ptr(), V,
                                                float(tiou), rec.data_ptr(), prc.data_ptr(), best.data_ptr(), ops.stream_ptr()),
               "hirest_step_bound_pr")
    return rec, prc, best


def preprocess_bounds(preds: torch.Tensor, pred_off: torch.Tensor, gt_minmax: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (bounds [V,max_out,2] float64, count [V] int32)."""
    V = pred_off.numel() - 1
    dev = preds.device
    counts_in = (pred_off[1:] - pred_off[:-1])
    max_in = int(counts_in.max().item()) if V else 0
    if max_in > 128:
        raise ValueError("at most 128 predicted bounds per video")
    max_out = 2 * max_in + 1
    out = torch.zeros((V, max_out, 2), dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().hirest_preprocess_moment_bounds(preds.data_ptr(), pred_off.data_ptr(), gt_minmax.data_ptr(), V,
                                                           out.data_ptr(), cnt.data_ptr(), max_out, ops.stream_ptr()),
               "hirest_preprocess_moment_bounds")
    return out, cnt


def _ragged(lists: Sequence[Sequence[Sequence[float]]], device):
    flat, off = [], [0]
    for l in lists:
        flat.extend([float(b[0]), float(b[1])] for b in l)
        off.append(len(flat))
    t = torch.tensor(flat if flat else [[0.0, 0.0]], dtype=torch.float64).reshape(-1, 2)[: len(flat)]
    return t.to(device).contiguous(), torch.tensor(off, dtype=torch.int32, device=device)


# ------------------------------------------------------------------------------------------------ evaluate.py level

def evaluate_video_retrieval(gt_data, pred_data, prompt_to_cat: Optional[Dict[str, str]] = None, device=None,
                             ks: Sequence[int] = (1, 5, 10, 50)) -> dict:
    """evaluate.py:33-81.  ``pred`` is the retrieval script's dict ``{prompt: {"videos": [...], "scores": [...]}}`` (a path, a
    plain dict, or the ``RetrievalResult`` of ``retrieval.run_corpus``, whose device-resident score matrix is then ranked
    in place).  The reference sorts ``zip(scores, videos)`` ascending and reverses: score descending, exact ties broken by
    file name descending; here that order is one top-``max(ks)`` selection per prompt on the device (``hirest_topk_f32`` with
    the name ranks as tie key), and only the ``[Q, max(ks)]`` index table comes back for the membership test.  Prompts whose
    ``videos`` lists differ are ranked in groups sharing a list.  ``prompt_to_cat`` None: only the 'all' bucket."""
    from . import retrieval
    gt, pred = _load(gt_data), _load(pred_data)
    device = _dev(device)
    cat_of = prompt_to_cat or {}
    cats = _categories(cat_of)
    ks = [int(k) for k in ks]
    count = {c: {str(k): 0 for k in ks} for c in cats}
    total = {c: 0 for c in cats}
    prompts = list(gt)
    # group prompts by the identity / content of their video list (the script writes one shared list)
    by_id: Dict[int, Tuple[List[str], List[str]]] = {}
    groups: Dict[tuple, Tuple[List[str], List[str]]] = {}
    for p in prompts:
        vids = pred[p]["videos"]
        g = by_id.get(id(vids))
        if g is None:
            g = by_id[id(vids)] = groups.setdefault(tuple(vids), (list(vids), []))
        g[1].append(p)
    whole = getattr(pred, "scores", None)
    for vids, members in groups.values():
        kmax = min(max(ks), len(vids))
        if whole is not None and vids == getattr(pred, "video_ids", None) and members == getattr(pred, "prompts", None):
            scores = whole.to(device)
        else:
            scores = torch.tensor([pred[p]["scores"] for p in members], dtype=torch.float32, device=device)
        _, idx = ops.topk(scores.contiguous(), kmax, retrieval.tie_rank_from_names(vids, device))
        idx = idx.cpu().tolist()
        for p, row in zip(members, idx):
            gt_videos = set(gt[p].keys()) if isinstance(gt[p], dict) else set(gt[p])     # (the split files hold {video: annotation} dicts)
            buckets = ["all"] + ([cat_of[p]] if prompt_to_cat is not None else [])
            for c in buckets:
                total[c] += 1
            for k in ks:
                if any(vids[v] in gt_videos for v in row[:k]):
                    for c in buckets:
                        count[c][str(k)] += 1
    results = {}
    for c in cats:
        if total[c] > 0:
            results[c] = {"total_prompt_count": total[c]}
            for k in ks:
                results[c][f"R@{k}"] = (count[c][str(k)] / total[c]) * 100
    return results


def evaluate_moment_retrieval(gt_data, pred_data, prompt_to_cat: Dict[str, str], device=None) -> dict:
    gt, pred = _load(gt_data), _load(pred_data)
    device = _dev(device)
    cats = _categories(prompt_to_cat)
    keys = [(p, v) for p in gt for v in gt[p] if gt[p][v]["clip"]]
    score_dict = {c: {} for c in cats}
    if not keys:
        return score_dict
    g = torch.tensor([[float(x) for x in gt[p][v]["bounds"][:2]] for p, v in keys], dtype=torch.float64, device=device)
    q = torch.tensor([[float(x) for x in pred[p][v]["bounds"][:2]] for p, v in keys], dtype=torch.float64, device=device)
    iou = interval_iou(g, q)
    for tiou in (0.5, 0.7):
        hit = (~(iou < tiou)).cpu().tolist()                        # score = 0 if iou < tIoU else 1
        scores = {c: [] for c in cats}
        for (p, _), h in zip(keys, hit):
            scores["all"].append(int(h))
            scores[prompt_to_cat[p]].append(int(h))
        for c in cats:
            if len(scores[c]) > 0:
                score_dict[c]["total_videos"] = len(scores[c])
                score_dict[c][f"R@{tiou}"] = sum(scores[c]) / len(scores[c]) * 100
    return score_dict


def compute_step_bound_scores(gt_data, pred_data, video_to_cat: Dict[str, str], device=None) -> dict:
    gt, pred = _load(gt_data), _load(pred_data)
    device = _dev(device)
    cats = _categories(video_to_cat)
    videos = list(gt)
    results = {c: {"recall": {}, "precision": {}} for c in cats}
    for v in videos:
        if len(pred[v]["bounds"]) == 0 or len(gt[v]["bounds"]) == 0:
            raise ValueError(f"{v}: empty bounds list (the reference divides by the list length)")
    refs, ref_off = _ragged([gt[v]["bounds"] for v in videos], device)
    preds, pred_off = _ragged([pred[v]["bounds"] for v in videos], device)
    for tiou in (0.5, 0.7):
        rec, prc, _ = step_bound_pr(refs, ref_off, preds, pred_off, tiou)
        rec, prc = rec.cpu().tolist(), prc.cpu().tolist()
        recall = {c: [] for c in cats}
        precision = {c: [] for c in cats}
        for v, r, p in zip(videos, rec, prc):
            for c in (video_to_cat[v], "all"):
                recall[c].append(r)
                precision[c].append(p)
        for c in cats:
            if len(recall[c]) > 0:
                results[c]["recall"][f"{tiou}"] = sum(recall[c]) / len(recall[c]) * 100
                results[c]["precision"][f"{tiou}"] = sum(precision[c]) / len(precision[c]) * 100
                results[c]["total"] = len(recall[c])
    return results


def preprocess_moment_bounds(gt_data, pred_data, device=None) -> dict:
    gt, pred = _load(gt_data), _load(pred_data)
    device = _dev(device)
    videos = list(pred)
    preds, pred_off = _ragged([pred[v]["bounds"] for v in videos], device)
    mm = torch.tensor([[float(gt[v]["bounds"][0][0]), float(gt[v]["bounds"][-1][1])] for v in videos], dtype=torch.float64,
                      device=device)
    out, cnt = preprocess_bounds(preds, pred_off, mm)
    out, cnt = out.cpu(), cnt.cpu().tolist()
    res = {}
    for i, v in enumerate(videos):
        res[v] = dict(pred[v])
        res[v]["bounds"] = out[i, : cnt[i]].tolist()
    return res


# ------------------------------------------------------------------------------------------------ CLIPScore (step captioning)

CLIP_SCORE_FRAMES = 4            # evaluate.py:241: np.linspace(start, end - 1, 4)
CLIP_SCORE_CHUNK = 1024          # unique frames decoded and encoded per round (1024 frames at 360p: 0.7 GB decoded)
TEXT_BATCH = 1024


def _no_frames(frame_dir) -> bool:
    return frame_dir is None or str(frame_dir) == "None"


def _frame_files(frame_dir, video: str) -> List[str]:
    """evaluate.py:236-237, verbatim: glob, then the integer after the last '_' of the whole path."""
    from glob import glob
    frames = glob(f"{frame_dir}/{video}/*.jpg")
    frames.sort(key=lambda a: int(a.split("_")[-1].replace(".jpg", "")))
    return frames


def _caption_plan(gt: dict, pred: dict, video_to_cat: Optional[Dict[str, str]], per_category: bool,
                  videos: Optional[Sequence[str]] = None):
    """What evaluate_moment_summarization's loops (evaluate.py:212-291) decide for every model-based caption metric, host only:
    ``(order, captions, candidates, references, categories)`` — the GT videos walked, every (video, caption index) in loop order,
    the lower-cased predicted and GT sentence of each (:233-234), and ``{category: {"Total": matching videos, "captions": indices
    into captions}}`` in ``_categories`` order without the categories that have no caption (:290-291).  ``video_to_cat[video]`` is
    looked up for every GT video (:225: a missing one raises KeyError); None: only "all", no lookups."""
    if videos is None:
        order = list(gt)
    else:
        wanted = set(videos)
        missing = wanted - set(gt)
        if missing:
            raise KeyError(f"videos not in the GT data: {sorted(missing)[:5]}")
        order = [v for v in gt if v in wanted]
    cats = _categories(video_to_cat) if (per_category and video_to_cat is not None) else ["all"]
    members = {c: [] for c in cats}
    totals = {c: 0 for c in cats}
    captions, candidates, references = [], [], []
    for video in order:
        video_cat = video_to_cat[video] if video_to_cat is not None else None     # evaluate.py:219, KeyError like VIDEOS_TO_CAT
        mine = [c for c in cats if c == "all" or c == video_cat]
        for c in mine:
            totals[c] += 1
        for i, d in enumerate(gt[video]["captions"]):
            for c in mine:
                members[c].append(len(captions))
            captions.append((video, i))
            references.append(d["sentence"].lower())
            candidates.append(pred[video]["captions"][i]["sentence"].lower())
    categories = {c: {"Total": totals[c], "captions": members[c]} for c in cats if members[c]}
    return order, captions, candidates, references, categories


class ClipScorePlan:
    """Host-side selection of a CLIPScore run (see ``clip_score_plan``).

    captions    every (video, caption index) of the selected GT videos, in evaluate.py's loop order
    candidates  the candidate sentence of each caption, lower-cased
    skip        per caption: True when it gets no score
    scored      indices into ``captions`` of the scored ones, in order (C of them)
    sel         int32 [C, 4]: rows of ``frames`` that feed each scored caption, in linspace order (repeats kept)
    frames      the unique frame files (U), in order of first use
    tokens      int64 [C, 77] CPU: clip.tokenize of the scored candidates (truncate=False)
    categories  {category: {"Total": matching videos, "captions": indices into ``captions``}} for the categories evaluate.py
                reports, in ``_categories`` order
    """

    def __init__(self, captions, candidates, skip, scored, sel, frames, tokens, categories):
        self.captions, self.candidates, self.skip, self.scored = captions, candidates, skip, scored
        self.sel, self.frames, self.tokens, self.categories = sel, frames, tokens, categories


def clip_score_plan(gt_data, pred_data, frame_dir, video_to_cat: Optional[Dict[str, str]] = None, per_category: bool = False,
                    videos: Optional[Sequence[str]] = None, context_length: int = 77) -> ClipScorePlan:
    """Everything evaluate_moment_summarization (evaluate.py:190-320) decides about CLIPScore before the model runs; host only.

    * categories: ``per_category`` false -> only "all" (evaluate.py:490-491), else those of ``video_to_cat`` plus "all"; a category
      none of whose matching videos has a caption is left out (:290-291).  ``video_to_cat[video]`` is looked up for every GT video
      (:219), so a missing video raises KeyError.  ``video_to_cat`` None: only "all", no lookups (the per-caption form).
    * "Total" counts the matching videos (:222-223), not the captions.
    * candidate: ``pred[video]["captions"][i]["sentence"].lower()`` (:228); the GT sentence plays no part.  It is tokenized with
      truncate=False (:243), so a scored candidate of more than 77 tokens raises RuntimeError.
    * frames: ``glob(f"{frame_dir}/{video}/*.jpg")`` sorted by ``int(path.split("_")[-1].replace(".jpg", ""))`` (:235-237); GT keys
      carry ".mp4", so that is the directory name.  Listed once per video (the reference re-lists per caption: the same list).
    * skip: ``start >= n_frames or end >= n_frames`` (:239-241); a missing directory has n_frames = 0 and skips every caption.
    * frame indices: ``np.linspace(start, min(end, n) - 1, 4).astype(int)`` in float64 (:244), applied to the frame array as numpy
      indexing does (a negative index counts from the end, as for a one-frame segment start == end); repeats stay.
    * ``frame_dir`` None or "None": nothing is scored (the guard at :204,236), every category present reports CLIPScore 0.
    """
    from .tokenizer import tokenize
    gt, pred = _load(gt_data), _load(pred_data)
    no_frames = _no_frames(frame_dir)
    order, captions, candidates, _, categories = _caption_plan(gt, pred, video_to_cat, per_category, videos)
    skip, scored, sel_rows = [], [], []
    frames, row_of = [], {}
    k = 0
    for video in order:
        files = None
        for i, d in enumerate(gt[video]["captions"]):
            k += 1
            if no_frames:
                skip.append(True)
                continue
            if files is None:
                files = _frame_files(frame_dir, video)
            n = len(files)
            if d["start"] >= n or d["end"] >= n:
                skip.append(True)
                continue
            skip.append(False)
            idxes = np.linspace(d["start"], min(d["end"], n) - 1, CLIP_SCORE_FRAMES).astype(int)
            row = []
            for f in np.array(files)[idxes]:
                f = str(f)
                if f not in row_of:
                    row_of[f] = len(frames)
                    frames.append(f)
                row.append(row_of[f])
            scored.append(k - 1)
            sel_rows.append(row)
    sel = np.array(sel_rows, dtype=np.int32).reshape(len(sel_rows), CLIP_SCORE_FRAMES)
    tokens = tokenize([candidates[k] for k in scored], context_length=context_length, truncate=False)
    return ClipScorePlan(captions, candidates, skip, scored, sel, frames, tokens, categories)


def _model_device(model, device):
    if device is None:
        device = next(model.parameters()).device
    return _dev(device)


@torch.no_grad()
def _plan_scores(plan: ClipScorePlan, model, device, chunk: int = CLIP_SCORE_CHUNK, stats: Optional[dict] = None) -> np.ndarray:
    """The device pipeline of a plan -> float32 [C] scores (host).  Unique frames go in chunks of at most ``chunk``: read, decoded
    (jpeg.Decoder), resized + cropped per geometry (FramePreprocessor), encoded (CLS head) into one [U, E] buffer; the candidates are
    encoded in batches of TEXT_BATCH; one hirest_clip_score launch scores every caption.  ``stats`` (a dict): filled with counts,
    the host-decoded files, and per-stage seconds (each stage is then synchronised, which costs a little overlap)."""
    import time
    from . import jpeg
    from .features import _prepare_frames
    C, U = len(plan.scored), len(plan.frames)
    if C == 0:
        return np.zeros(0, np.float32)
    timed = stats is not None
    t = {k: 0.0 for k in ("read_s", "decode_s", "preprocess_s", "image_tower_s", "text_tower_s", "score_s")}
    fallbacks = []

    def mark(key, t0):
        if timed:
            torch.cuda.synchronize(device)
            t[key] += time.perf_counter() - t0
        return time.perf_counter()
    decoder = jpeg.Decoder()
    emb = None
    with torch.cuda.device(device):
        t0 = time.perf_counter()
        for s in range(0, U, max(1, int(chunk))):
            files = plan.frames[s:s + chunk]
            blobs = jpeg._pool_map(jpeg._read, files)
            t0 = mark("read_s", t0)
            dec = decoder.decode(blobs, device)
            fallbacks.extend((files[i], why) for i, why in decoder.last_fallbacks)
            t0 = mark("decode_s", t0)
            if isinstance(dec, torch.Tensor):
                groups = [(None, dec)]
            else:
                by_shape = {}
                for i, f in enumerate(dec):
                    by_shape.setdefault(tuple(f.shape), []).append(i)
                groups = [(ids, torch.stack([dec[i] for i in ids])) for ids in by_shape.values()]
            for ids, frames in groups:
                x = _prepare_frames(model, frames)
                t0 = mark("preprocess_s", t0)
                out = model.encode_image(x)
                if out.dim() != 2:
                    raise ValueError("CLIPScore needs the CLS embedding of the pip `clip` package: load the model with pip_head=True")
                if emb is None:
                    emb = torch.empty((U, out.shape[1]), dtype=torch.float32, device=device)
                if ids is None:
                    emb[s:s + out.shape[0]] = out
                else:
                    emb[torch.tensor(ids, device=device) + s] = out.float()
                t0 = mark("image_tower_s", t0)
            del dec, groups
        tok = plan.tokens.to(device)
        txt = torch.cat([model.encode_text(tok[b:b + TEXT_BATCH]).float() for b in range(0, C, TEXT_BATCH)])
        t0 = mark("text_tower_s", t0)
        scores = ops.clip_score(emb, txt, torch.from_numpy(plan.sel))
        t0 = mark("score_s", t0)
        host = scores.cpu().numpy()                      # the one device -> host read of the scores
    if timed:
        stats.update(t)
        stats.update(captions=len(plan.captions), scored=C, unique_frames=U, fallbacks=fallbacks)
    return host


def caption_clip_scores(gt_data, pred_data, model, frame_dir, videos: Optional[Sequence[str]] = None, device=None,
                        stats: Optional[dict] = None) -> List[Tuple[str, int, Optional[float]]]:
    """Per-caption CLIPScore of evaluate.py:204-262: ``[(video, caption_index, score or None), ...]`` in the reference's loop
    order; None marks a skipped caption (see ``clip_score_plan`` for the rules).  ``model``: ``clip.load(..., pip_head=True)``."""
    plan = clip_score_plan(gt_data, pred_data, frame_dir, videos=videos)
    vals = _plan_scores(plan, model, _model_device(model, device), stats=stats) if plan.scored else []
    out: List[Tuple[str, int, Optional[float]]] = [(v, i, None) for v, i in plan.captions]
    for k, s in zip(plan.scored, vals):
        out[k] = (plan.captions[k][0], plan.captions[k][1], float(s))
    return out


def evaluate_clip_score(gt_data, pred_data, video_to_cat: Dict[str, str], model, frame_dir, per_category: bool = False,
                        device=None, stats: Optional[dict] = None) -> dict:
    """The CLIPScore leg of evaluate_moment_summarization (evaluate.py:190-320): ``{category: {"CLIPScore": float, "Total": int}}``.

    The selection rules are ``clip_score_plan``'s.  Every unique frame is decoded and encoded once, every candidate once, and one
    kernel launch scores all captions; ``CLIPScore`` is ``np.average`` of a category's per-caption Python floats in the reference's
    order, 0 when it has none (:303-304).  ``model`` is ``hirest_amd.clip.load(..., pip_head=True)``, used at whatever precision the
    caller set.  The reference runs the pip ``clip`` model in fp16 on CUDA (``clip.load`` applies ``convert_weights`` and casts back
    to fp32 only on CPU); no precision here reproduces its numbers bit for bit, and ``precision='fp32'`` is the recommended setting
    for reporting."""
    plan = clip_score_plan(gt_data, pred_data, frame_dir, video_to_cat, per_category)
    vals = _plan_scores(plan, model, _model_device(model, device), stats=stats) if plan.scored else []
    score_of = {k: float(s) for k, s in zip(plan.scored, vals)}
    results = {}
    for c, m in plan.categories.items():
        clip_scores = [score_of[k] for k in m["captions"] if k in score_of]
        if len(clip_scores) == 0:
            clip_scores = [0]
        results[c] = {"CLIPScore": float(np.average(clip_scores)), "Total": m["Total"]}
    return results


def evaluate_bert_score(gt_data, pred_data, video_to_cat: Dict[str, str], scorer, per_category: bool = False, device=None,
                        stats: Optional[dict] = None) -> dict:
    """The BERTScore leg of evaluate_moment_summarization (evaluate.py:190-320): ``{category: {"BERTScore_F1": float, "Total": int}}``.

    Categories, their order, ``Total`` and the rule that drops a category without captions are ``clip_score_plan``'s (one shared
    walk of the GT videos).  Per caption the pair is (predicted sentence, GT sentence), both lower-cased (:233-234).  ``scorer`` is a
    ``hirest_amd.bert_score.BERTScorer``: every unique sentence is encoded once, one ``hirest_bertscore_greedy`` launch scores all
    pairs of all categories, and a category's figure is ``f.mean().item()`` of the fp32 F of its pairs in loop order (:308)."""
    gt, pred = _load(gt_data), _load(pred_data)
    _, captions, candidates, references, categories = _caption_plan(gt, pred, video_to_cat, per_category)
    if not captions:
        return {}
    if device is not None:
        scorer.to(_dev(device))
    f = scorer.score_device(candidates, references, stats=stats)[:, 2].cpu()          # the one device -> host read
    return {c: {"BERTScore_F1": f[torch.tensor(m["captions"])].mean().item(), "Total": m["Total"]} for c, m in categories.items()}
