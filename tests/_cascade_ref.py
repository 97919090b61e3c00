"""Pure-Python restatement of the three seams of the end-to-end cascade (csrc/cascade.hip), built from pieces that are pinned
elsewhere: ``timeline.frame_index_to_timestamp`` / ``timestamp_to_frame_index`` (tests/test_timeline.py, against the reference),
the list logic of ``MomentModel.test_moment_segmentation`` and ``MomentModel._trim_index`` (tests/test_gpu_joint.py, against the
reference).  tests/test_cascade_host.py checks it against the real reference's chain (tests/golden/cascade_a.*); the GPU tests
compare the kernels with it.  Not a test module."""
from hirest_amd.moment_model import MomentModel
from hirest_amd.timeline import frame_index_to_timestamp, timestamp_to_frame_index


def moment_bounds(pred, duration, n_frames, T):
    """Seam (a) for one sample: (bounds_ts, bound_frames, moment_mask, boundary_mask)."""
    ts = [frame_index_to_timestamp(f, duration, n_frames) for f in pred]
    fr = [timestamp_to_frame_index(t, duration, n_frames) for t in ts]
    mm, bm = [0] * T, [0] * T
    mm[fr[0]:fr[1] + 1] = [1] * len(mm[fr[0]:fr[1] + 1])
    bm[fr[0]] = 1
    return ts, fr, mm, bm


def boundary_list(steps, start, last):
    """The post-processing of test_moment_segmentation (hirest_amd/moment_model.py, modeling.py:435-463) for one sample."""
    sp = [[start, start]] + [list(s) for s in steps] + [[last, last]]
    sp.sort(key=lambda x: x[0])
    flat = [v for s in sp for v in s]
    while flat[-1] > last:
        flat.pop(-1)
    temp = sorted(set(flat))
    keep, cur = [temp[0]], temp[0]
    for i in range(1, len(temp) - 1):
        if temp[i] - cur >= 5:
            keep.append(temp[i])
            cur = temp[i]
    return keep


def steps_of(bounds, duration, n_frames):
    """Seam (b), step level, for one sample: (step_ts, step_frames)."""
    ts = [[frame_index_to_timestamp(bounds[j], duration, n_frames), frame_index_to_timestamp(bounds[j + 1], duration, n_frames)]
          for j in range(len(bounds) - 1)]
    fr = [[timestamp_to_frame_index(t, duration, n_frames) for t in pair] for pair in ts]
    return ts, fr


def boundaries(steps, nsteps, bound_frames, durations, n_frames):
    """Seam (b) for a batch: dict with n_bounds, bounds (ragged), step_ts, step_frames, step_sample, offsets."""
    out = {"n_bounds": [], "bounds": [], "step_ts": [], "step_frames": [], "step_sample": [], "offsets": [0]}
    for b in range(len(nsteps)):
        nf = n_frames if isinstance(n_frames, int) else n_frames[b]
        keep = boundary_list(steps[b][:nsteps[b]], bound_frames[b][0], bound_frames[b][1])
        ts, fr = steps_of(keep, durations[b], nf)
        out["n_bounds"].append(len(keep))
        out["bounds"].append(keep)
        out["step_ts"] += ts
        out["step_frames"] += fr
        out["step_sample"] += [b] * len(ts)
        out["offsets"].append(len(out["step_ts"]))
    return out


def caption_mask(a, e, T):
    """hirest_dataset.py:302-304: ``mask[a:e] = 1; mask[e] = 1``."""
    m = [0] * T
    m[a:e] = [1] * len(m[a:e])
    m[e] = 1
    return m


def trim_rows(a, e, T, max_frames):
    """Seam (c): the frame each of the max_frames slots of step (a, e) takes."""
    return MomentModel._trim_index(caption_mask(a, e, T), max_frames)
