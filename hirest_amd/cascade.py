"""End-to-end cascade of the joint model's three tasks (the reference's ``run.py --end_to_end``, run.py:383-490).

The reference chains moment retrieval -> moment segmentation -> step captioning through ``all_data_test.json``: each stage's
predictions are written into the file and the next stage's ``MomentDataset`` is rebuilt from it (hirest_dataset.py:186-311).
Here the features go to the device once, the text is encoded once, and the seams are three small kernels (csrc/cascade.hip):

    retrieval  --hirest_cascade_moment_bounds-->  segmentation  --hirest_cascade_boundaries-->  steps
               --hirest_cascade_trim_gather-->    caption decoder inputs  -->  merged beam search

What the seams reproduce, integer for integer:
  * frames -> seconds -> frames: run.py:731-732 writes ``frame_index_to_timestamp`` of the arg-max frames; the segmentation dataset
    re-quantises them with ``timestamp_to_frame_index`` (hirest_dataset.py:250-254), which is not the identity when the number of
    model frames differs from the duration.  The same happens to every step boundary (run.py:766-770, hirest_dataset.py:289-290).
  * the segmentation mask is ``mask[start : end + 1]`` (hirest_dataset.py:259-260), the captioning mask ``mask[start : end]`` plus
    ``mask[end] = 1`` (hirest_dataset.py:302-304): the same frames when start <= end, but frame ``end`` alone when start > end.
  * the segmentation's post-processing never emits its last boundary (modeling.py:458).

The host sees one ``[B + 1]`` copy per batch — the step offsets, whose last entry sizes the captioning buffers — and reads every
result out after the captions are done.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Sequence

import torch

from . import _lib, ops

_BAD = -(1 << 63)


def _n_frames_arg(model, batch, B, dev):
    nf = batch.get("n_frames")
    if nf is None:
        nf = model.n_frames if isinstance(model.n_frames, int) and model.n_frames > 0 else -1
    if isinstance(nf, int):
        return None, int(nf)
    t = torch.as_tensor(nf).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if t.numel() != B:
        raise ValueError(f"{B} samples but {t.numel()} n_frames")
    return t, 0


def moment_bounds(pred_frames: torch.Tensor, durations: torch.Tensor, n_frames, n_frames_all: int, T: int):
    """Seam (a).  pred_frames int32 [B,2], durations float64 [B] (device) -> bounds_ts int64 [B,2], bound_frames int32 [B,2],
    moment_mask int32 [B,T], boundary_mask int32 [B,T]."""
    dev, B = pred_frames.device, pred_frames.shape[0]
    ts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    fr = torch.empty((B, 2), dtype=torch.int32, device=dev)
    mm = torch.empty((B, T), dtype=torch.int32, device=dev)
    bm = torch.empty((B, T), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().hirest_cascade_moment_bounds(pred_frames.data_ptr(), durations.data_ptr(),
                                                        n_frames.data_ptr() if n_frames is not None else None, n_frames_all, B, T,
                                                        ts.data_ptr(), fr.data_ptr(), mm.data_ptr(), bm.data_ptr(), ops.stream_ptr()),
               "hirest_cascade_moment_bounds")
    return ts, fr, mm, bm


def boundaries(steps: torch.Tensor, nsteps: torch.Tensor, bound_frames: torch.Tensor, durations: torch.Tensor, n_frames,
               n_frames_all: int) -> Dict[str, torch.Tensor]:
    """Seam (b).  steps int32 [B,iters,2], nsteps int32 [B], bound_frames int32 [B,2] -> n_bounds [B], bounds [B, 2 iters + 4],
    step_ts int64 [B (cap - 1), 2], step_frames int32 [.., 2], step_sample int32 [..], offsets int32 [B + 1] (all on the device; the
    step buffers are valid up to row offsets[B])."""
    dev, B, iters = steps.device, steps.shape[0], steps.shape[1]
    cap = 2 * iters + 4
    rows = max(B * (cap - 1), 1)
    out = {"n_bounds": torch.empty((B,), dtype=torch.int32, device=dev), "bounds": torch.empty((B, cap), dtype=torch.int32, device=dev),
           "step_ts": torch.empty((rows, 2), dtype=torch.int64, device=dev), "step_frames": torch.empty((rows, 2), dtype=torch.int32, device=dev),
           "step_sample": torch.empty((rows,), dtype=torch.int32, device=dev), "offsets": torch.empty((B + 1,), dtype=torch.int32, device=dev)}
    _lib.check(_lib.load().hirest_cascade_boundaries(steps.data_ptr(), nsteps.data_ptr(), bound_frames.data_ptr(), durations.data_ptr(),
                                                     n_frames.data_ptr() if n_frames is not None else None, n_frames_all, B, iters,
                                                     out["n_bounds"].data_ptr(), out["bounds"].data_ptr(), out["step_ts"].data_ptr(),
                                                     out["step_frames"].data_ptr(), out["step_sample"].data_ptr(),
                                                     out["offsets"].data_ptr(), ops.stream_ptr()), "hirest_cascade_boundaries")
    return out


def trim_gather(vis: torch.Tensor, asr, step_frames: torch.Tensor, step_sample: torch.Tensor, S: int, max_frames: int):
    """Seam (c).  vis fp32 [B,T,D] (asr fp32 [B,T,Da] or None) -> [S, max_frames, D] (and [S, max_frames, Da] or None)."""
    B, T, D = vis.shape
    out_v = torch.empty((S, max_frames, D), dtype=torch.float32, device=vis.device)
    out_a = torch.empty((S, max_frames, asr.shape[2]), dtype=torch.float32, device=vis.device) if asr is not None else None
    _lib.check(_lib.load().hirest_cascade_trim_gather(vis.data_ptr(), asr.data_ptr() if asr is not None else None, step_frames.data_ptr(),
                                                      step_sample.data_ptr(), S, B, T, D, asr.shape[2] if asr is not None else 0, max_frames,
                                                      out_v.data_ptr(), out_a.data_ptr() if out_a is not None else None, ops.stream_ptr()),
               "hirest_cascade_trim_gather")
    return out_v, out_a


def _stages(model, batch):
    """Retrieval, seam (a), segmentation, seam (b), seam (c) for one loader batch.  Everything stays on the device but the step
    offsets.  Returns the device state the read-out needs and the captioning inputs (None when the batch has no step)."""
    lib = _lib.load()
    dev = model._w()["dev"]
    vis = batch["vis_feats"].to(dev).float().contiguous()
    vmask, mmask = batch["vis_mask"].to(dev), batch["moment_mask"].to(dev)
    asr = batch["asr_feats"].to(dev).float().contiguous() if model.use_asr else None
    text = model._text_feat(batch, dev)                              # once, for all three stages
    B, T = vmask.shape
    if "video_duration" not in batch:
        raise KeyError("end_to_end needs batch['video_duration'] (the loader's collate_fn delivers it: hirest_dataset.py:522)")
    dur = torch.as_tensor(batch["video_duration"], dtype=torch.float64).reshape(-1).to(dev)
    if dur.numel() != B:
        raise ValueError(f"{B} samples but {dur.numel()} video durations")
    nf, nf_all = _n_frames_arg(model, batch, B, dev)
    args = model.args
    thr = float(getattr(args, "moment_segmentation_difference_threshold", 0.5)) if args is not None else 0.5
    iters = int(getattr(args, "moment_segmentation_max_iterations", 20)) if args is not None else 20
    max_frames = int(getattr(args, "max_frames_step_captioning", 20)) if args is not None else 20
    st = ops.stream_ptr()
    # the fusion's loop-invariant part is the same for retrieval and segmentation (same features, text, ASR, video mask)
    base = model._fusion_base(vis, text, asr, vmask)
    # --- moment retrieval (modeling.py:272-310)
    feats = model._features(base, mmask.to(torch.int32).contiguous(), None, B, T)
    lg = model._heads(feats, ["start", "end"])
    m32 = vmask.to(torch.int32).contiguous()
    pred = torch.empty((2, B), dtype=torch.int32, device=dev)
    for i in range(2):
        _lib.check(lib.hirest_masked_argmax(lg[i].contiguous().data_ptr(), m32.data_ptr(), -1e10, B, T, pred[i].data_ptr(), st),
                   "hirest_masked_argmax")
    pred = pred.t().contiguous()                                     # [B, 2]
    # --- seam (a)
    bounds_ts, bound_frames, mm, bm = moment_bounds(pred, dur, nf, nf_all, T)
    # --- moment segmentation (modeling.py:353-433): the loop of test_moment_segmentation
    steps = torch.zeros((B, iters, 2), dtype=torch.int32, device=dev)
    nsteps = torch.zeros((B,), dtype=torch.int32, device=dev)
    for _ in range(iters):
        f = model._features(base, mm, bm, B, T)
        logits = model._heads(f, ["segment"])[0].contiguous()
        _lib.check(lib.hirest_segmentation_step(logits.data_ptr(), mm.data_ptr(), bm.data_ptr(), B, T, thr, steps.data_ptr(),
                                                nsteps.data_ptr(), iters, None, st), "hirest_segmentation_step")
    # --- seam (b); its offsets are the one device -> host copy in front of the captioning stage
    sb = boundaries(steps, nsteps, bound_frames, dur, nf, nf_all)
    offsets = sb["offsets"].cpu().tolist()
    S = offsets[-1]
    state = {"B": B, "pred": pred, "bounds_ts": bounds_ts, "n_bounds": sb["n_bounds"], "bounds": sb["bounds"],
             "step_ts": sb["step_ts"][:S], "offsets": offsets, "S": S}
    cap_in = None
    if S > 0:
        # --- seam (c)
        v, a = trim_gather(vis, asr, sb["step_frames"], sb["step_sample"], S, max_frames)
        cap_in = (v, a, text.index_select(0, sb["step_sample"][:S].long()))
    return state, cap_in


def _read_out(state, captions: List) -> Dict[str, List]:
    B, off = state["B"], state["offsets"]
    pred, bts = state["pred"].cpu().tolist(), state["bounds_ts"].cpu().tolist()
    nb, bd = state["n_bounds"].cpu().tolist(), state["bounds"].cpu().tolist()
    sts = state["step_ts"].cpu().tolist()
    if any(v == _BAD for row in bts for v in row):
        raise IndexError("a retrieved frame index lies outside its video's bins (check video_duration / n_frames)")
    out = {"moment_frames": pred, "bounds": bts, "boundary_frames": [bd[b][:nb[b]] for b in range(B)], "step_bounds": [], "captions": []}
    for b in range(B):
        out["step_bounds"].append(sts[off[b]:off[b + 1]])
        out["captions"].append(list(captions[off[b]:off[b + 1]]))
    return out


@torch.no_grad()
def run_end_to_end(model, batches: Sequence[dict], num_beams: int = 5, return_ids: bool = False, rows_in_flight=None) -> List[Dict[str, List]]:
    """``MomentModel.end_to_end`` over a list of moment-retrieval loader batches.  Each batch runs retrieval and segmentation on its
    own; the steps of consecutive batches are captioned by ONE merged beam search of up to ``rows_in_flight`` beam rows (default
    ``MomentModel.CAPTION_ROWS_IN_FLIGHT``), as ``caption_batches`` merges loader batches: every kernel behind the trim is
    batch-invariant, so a step's caption does not depend on what it is merged with.  Returns one result dict per batch, in order."""
    import contextlib
    batches = list(batches)
    dev = model._w()["dev"]
    cap_rows = max(1, int(rows_in_flight or model.CAPTION_ROWS_IN_FLIGHT) // max(1, num_beams))     # steps per merged search
    states, caps = [], []

    def caption(group):
        """One search over the steps of the batches in `group` (indices into states)."""
        ins = [caps[i] for i in group if caps[i] is not None]
        if not ins:
            return
        v = torch.cat([x[0] for x in ins], 0) if len(ins) > 1 else ins[0][0]
        a = None
        if model.use_asr:
            a = torch.cat([x[1] for x in ins], 0) if len(ins) > 1 else ins[0][1]
        t = torch.cat([x[2] for x in ins], 0) if len(ins) > 1 else ins[0][2]
        res = model._caption_trimmed(v, a, t, num_beams, return_ids)
        texts = res["token_ids"] if return_ids else res["prediction"]
        lo = 0
        for i in group:
            n = states[i]["S"]
            states[i]["captions"] = texts[lo:lo + n]
            lo += n
            caps[i] = None                                           # release the gathered rows

    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        group, rows = [], 0
        for batch in batches:
            state, cap_in = _stages(model, batch)
            states.append(state)
            caps.append(cap_in)
            i = len(states) - 1
            if group and rows + state["S"] > cap_rows:
                caption(group)
                group, rows = [], 0
            group.append(i)
            rows += state["S"]
        if group:
            caption(group)
        return [_read_out(s, s.get("captions", [])) for s in states]


def _heading(caption) -> str:
    return caption if isinstance(caption, str) else " ".join(map(str, caption))


def end_to_end_results(test_data: Dict, prompts: Sequence[str], video_fnames: Sequence[str], outputs) -> Dict:
    """The dict the reference writes to ``final_end_to_end_results.json`` (run.py:396-485): a copy of the split ``test_data``
    (``{prompt: {video: annotation}}``) in which every processed (prompt, video) has ``bounds`` replaced by the retrieved moment
    (run.py:409) and ``steps`` by ``[{"index": i, "heading": caption, "absolute_bounds": [s_i, s_i+1]}]`` (run.py:448-453, :480).

    ``prompts`` / ``video_fnames`` name the samples of ``outputs`` in order; ``outputs`` is one result dict of
    ``MomentModel.end_to_end`` or the list ``run_end_to_end`` returns.  Videos the loader skipped (not relevant, or without a clip:
    hirest_dataset.py:131-134) are left untouched — the reference also empties their ``steps`` (run.py:443), which HiREST's skipped
    videos do not have.  The reference keys its second and third stage by the video name alone (run.py:445, :478) and overwrites one
    prompt's steps with another's when a video is processed under two prompts; such input raises ValueError here."""
    if isinstance(outputs, dict):
        outputs = [outputs]
    flat = {k: [x for o in outputs for x in o[k]] for k in ("bounds", "step_bounds", "captions")}
    n = len(flat["bounds"])
    if not (len(prompts) == len(video_fnames) == n):
        raise ValueError(f"{n} samples in outputs but {len(prompts)} prompts and {len(video_fnames)} video names")
    seen = {}
    for p, v in zip(prompts, video_fnames):
        if v in seen:
            raise ValueError(f"video {v!r} is processed twice (under {seen[v]!r} and {p!r}): the reference keys its segmentation and "
                             "captioning results by the video name alone and would mix the two up")
        seen[v] = p
    out = copy.deepcopy(test_data)
    for i, (p, v) in enumerate(zip(prompts, video_fnames)):
        if p not in out or v not in out[p]:
            raise KeyError(f"({p!r}, {v!r}) is not in the split data")
        entry = out[p][v]
        entry["bounds"] = [int(x) for x in flat["bounds"][i]]
        if len(flat["captions"][i]) != len(flat["step_bounds"][i]):
            raise ValueError(f"sample {i}: {len(flat['step_bounds'][i])} steps but {len(flat['captions'][i])} captions")
        entry["steps"] = [{"index": j, "heading": _heading(c), "absolute_bounds": [int(x) for x in sb]}
                          for j, (sb, c) in enumerate(zip(flat["step_bounds"][i], flat["captions"][i]))]
    return out
