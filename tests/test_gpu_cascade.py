"""End-to-end cascade on the GPU: the three seam kernels (csrc/cascade.hip) against their pure-Python restatement
(tests/_cascade_ref.py, itself pinned to the real reference by tests/test_cascade_host.py) — integers equal, gathered rows
bit-equal — and MomentModel.end_to_end against three chained test_step calls and against the real reference's chain
(tests/golden/cascade_a.*)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cascade_ref as ref  # noqa: E402
import hirest_amd  # noqa: E402
from hirest_amd import cascade, synth  # noqa: E402
from hirest_amd.timeline import frame_index_to_timestamp, timestamp_to_frame_index  # noqa: E402

pytestmark = pytest.mark.gpu

# (T, duration): fewer seconds than frames, 37 s on 64 frames, 600 s on 300 frames
TIMELINES = [(7, 5), (64, 37), (300, 600)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------------------ seam (a)

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,duration", TIMELINES)
@pytest.mark.parametrize("per_sample", [False, True])
def test_moment_bounds(dev, B, T, duration, per_sample):
    # s = e, s > e, s = 0 with e = T - 1, and an ordinary pair; the frame -> second -> frame map is not the identity for (7, 5), (64, 37)
    cases = [[T // 2, T // 2], [T - 2, 1], [0, T - 1], [T // 3, 2 * T // 3], [T - 1, T - 1], [0, 0]]
    for lo in range(0, len(cases), B):
        pred = cases[lo:lo + B]
        if len(pred) < B:
            break
        durs = [duration + (b if per_sample else 0) for b in range(B)]
        nfs = [T - (b if per_sample and T > 7 else 0) for b in range(B)]
        pred = [[min(p[0], nfs[b] - 1), min(p[1], nfs[b] - 1)] for b, p in enumerate(pred)]
        ts, fr, mm, bm = cascade.moment_bounds(_i32(pred, dev), torch.tensor(durs, dtype=torch.float64, device=dev),
                                               _i32(nfs, dev) if per_sample else None, 0 if per_sample else T, T)
        assert ts.dtype == torch.int64 and fr.dtype == mm.dtype == bm.dtype == torch.int32
        for b in range(B):
            w_ts, w_fr, w_mm, w_bm = ref.moment_bounds(pred[b], durs[b], nfs[b], T)
            assert ts[b].tolist() == w_ts and fr[b].tolist() == w_fr
            assert mm[b].tolist() == w_mm and bm[b].tolist() == w_bm
            if pred[b][0] > pred[b][1] and w_fr[0] > w_fr[1]:
                assert sum(w_mm) == 0                                    # Python slice semantics: an empty moment


def test_moment_bounds_one_frame_per_second_and_errors(dev):
    lib = hirest_amd._lib.load()
    pred, durs = [[3, 30], [0, 11]], [40.0, 12.7]                        # n_frames < 0: int(duration) bins, one per second
    ts, fr, mm, bm = cascade.moment_bounds(_i32(pred, dev), torch.tensor(durs, dtype=torch.float64, device=dev), None, -1, 40)
    for b in range(2):
        w = ref.moment_bounds(pred[b], durs[b], -1, 40)
        assert (ts[b].tolist(), fr[b].tolist(), mm[b].tolist(), bm[b].tolist()) == w
    # a frame outside the bins: INT64_MIN / -1 and empty masks, never an out-of-bounds write
    ts, fr, mm, bm = cascade.moment_bounds(_i32([[2, 9]], dev), torch.tensor([5.0], dtype=torch.float64, device=dev), None, 7, 7)
    assert ts[0].tolist() == [frame_index_to_timestamp(2, 5.0, 7), -(1 << 63)] and fr[0].tolist() == [-1, -1] and int(mm.sum()) == 0 and int(bm.sum()) == 0
    assert lib.hirest_cascade_moment_bounds(None, None, None, 7, 1, 7, None, None, None, None, None) == -1
    assert lib.hirest_cascade_moment_bounds(1 << 20, 1 << 20, None, 7, 1, 0, 1 << 20, 1 << 20, 1 << 20, 1 << 20, None) == -1


# ------------------------------------------------------------------------------------------------------------ seam (b)

def _step_cases(T, iters):
    """(steps, start, last) triples: nsteps 0 / 1 / iters, duplicates, values above `last`, gaps of 4 / 5 / 6, a moment shorter than
    5 frames (a single boundary, zero steps), start > last."""
    l = T - 2
    full = [[1 + (3 * k) % (T - 2), min(T - 1, 2 + (3 * k) % (T - 2) + k % 4)] for k in range(iters)]
    c = [([], 0, l), ([[2, 4]], 1, l), (full, 1, l),
         ([[3, 5], [3, 5], [2, 5]], 1, l),                                # duplicates, and an equal key that must stay behind (stable)
         ([[2, T - 1], [3, 4]], 1, T - 3), ([[T - 2, T - 1]], 1, T - 3),  # above `last`: interior (kept in the set) and trailing (popped)
         ([], 2, 5), ([], 3, 3), ([], 4, 1)]                              # shorter than 5 frames; one frame; start > last
    if T >= 30:
        c += [([[5, 9], [14, 20]], 1, l), ([[5, 10], [15, 21]], 1, l), ([[5, 11], [17, 22]], 1, l)]      # gaps of 4, 5 and 6
    return c


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,duration", TIMELINES)
def test_boundaries(dev, B, T, duration):
    iters = 20
    cases = _step_cases(T, iters)
    cases += cases[:(-len(cases)) % B]
    for lo in range(0, len(cases), B):
        grp = cases[lo:lo + B]
        steps = torch.full((B, iters, 2), -7, dtype=torch.int32)          # entries past nsteps are never read
        for b, (st, _, _) in enumerate(grp):
            if st:
                steps[b, :len(st)] = torch.tensor(st, dtype=torch.int32)
        nsteps = [len(st) for st, _, _ in grp]
        bf = [[s, l] for _, s, l in grp]
        durs = [duration + b for b in range(B)]
        out = cascade.boundaries(steps.to(dev), _i32(nsteps, dev), _i32(bf, dev), torch.tensor(durs, dtype=torch.float64, device=dev),
                                 None, T)
        want = ref.boundaries(steps.tolist(), nsteps, bf, durs, T)
        S = want["offsets"][-1]
        assert out["offsets"].tolist() == want["offsets"] and out["n_bounds"].tolist() == want["n_bounds"]
        assert out["bounds"].shape == (B, 2 * iters + 4)
        for b in range(B):
            assert out["bounds"][b, :want["n_bounds"][b]].tolist() == want["bounds"][b]
            assert bool((out["bounds"][b, want["n_bounds"][b]:] == -1).all())
        assert out["step_ts"][:S].tolist() == want["step_ts"] and out["step_frames"][:S].tolist() == want["step_frames"]
        assert out["step_sample"][:S].tolist() == want["step_sample"]


def test_boundaries_many_samples_and_errors(dev):
    # more samples than one workgroup's four waves, ragged step counts: the offsets are a prefix sum over all earlier samples
    B, T, iters = 70, 64, 20
    g = torch.Generator().manual_seed(5)
    steps = torch.zeros((B, iters, 2), dtype=torch.int32)
    lo = torch.randint(1, T - 8, (B, iters), generator=g)
    steps[..., 0], steps[..., 1] = lo, lo + torch.randint(0, 7, (B, iters), generator=g)
    nsteps = [(3 * b) % (iters + 1) for b in range(B)]
    bf = [[b % 5, T - 1 - b % 7] for b in range(B)]
    durs = [37 + b for b in range(B)]
    out = cascade.boundaries(steps.to(dev), _i32(nsteps, dev), _i32(bf, dev), torch.tensor(durs, dtype=torch.float64, device=dev), None, T)
    want = ref.boundaries(steps.tolist(), nsteps, bf, durs, T)
    S = want["offsets"][-1]
    assert out["offsets"].tolist() == want["offsets"] and S > B
    assert [out["bounds"][b, :want["n_bounds"][b]].tolist() for b in range(B)] == want["bounds"]
    assert out["step_ts"][:S].tolist() == want["step_ts"] and out["step_frames"][:S].tolist() == want["step_frames"]
    assert out["step_sample"][:S].tolist() == want["step_sample"]
    lib = hirest_amd._lib.load()
    p = 1 << 20
    assert lib.hirest_cascade_boundaries(p, p, p, p, None, 64, 2, 31, p, p, p, p, p, p, None) == -2      # more than 64 values per sample
    assert lib.hirest_cascade_boundaries(p, None, p, p, None, 64, 2, 20, p, p, p, p, p, p, None) == -1


# ------------------------------------------------------------------------------------------------------------ seam (c)

@pytest.mark.parametrize("D,Da", [(1024, 384), (1024, 0), (8, 0), (8, 4)])
@pytest.mark.parametrize("B,T", [(1, 7), (3, 64), (3, 300)])
def test_trim_gather(dev, B, T, D, Da):
    F = 20
    # N = 1, 19, 20, 21, > 20 and a > e, as far as T allows
    spans = [(2, 2), (T - 1, T - 1), (0, min(T - 1, 18)), (1, min(T - 1, 20)), (0, min(T - 1, 20)), (3, min(T - 1, 60)), (5, 2), (T - 1, 0)]
    step_frames = [[a, e] for a, e in spans]
    step_sample = [(3 * i + 1) % B for i in range(len(spans))]
    S = len(spans)
    g = torch.Generator().manual_seed(T * 10 + D)
    vis = torch.randn((B, T, D), generator=g).to(dev)
    asr = torch.randn((B, T, Da), generator=g).to(dev) if Da else None
    # the buffers are larger than S, as the cascade's are: rows past S are never read
    sf = _i32(step_frames + [[-5, 10 ** 6]], dev)
    ss = _i32(step_sample + [10 ** 6], dev)
    v, a = cascade.trim_gather(vis, asr, sf, ss, S, F)
    assert v.shape == (S, F, D) and v.dtype == torch.float32 and (a is None) == (asr is None)
    idx = torch.tensor([ref.trim_rows(a_, e_, T, F) for a_, e_ in spans], device=dev)
    assert int(idx.min()) >= 0
    smp = torch.tensor(step_sample, device=dev)[:, None].expand(-1, F)
    assert torch.equal(v, vis[smp, idx])                                  # bit-equal rows
    if asr is not None:
        assert a.shape == (S, F, Da) and torch.equal(a, asr[smp, idx])


def test_trim_gather_invalid_steps_and_errors(dev):
    vis = torch.ones((2, 7, 8), device=dev)
    v, _ = cascade.trim_gather(vis, None, _i32([[0, 7], [1, 3], [-1, 2], [2, 3]], dev), _i32([0, 2, 0, 1], dev), 4, 20)
    assert v[:3].abs().sum().item() == 0 and bool((v[3] == 1).all())      # outside [0,B) x [0,T): zero rows, never a stray read
    lib = hirest_amd._lib.load()
    p = 1 << 20
    assert lib.hirest_cascade_trim_gather(p, None, p, p, 1, 1, 7, 6, 0, 20, p, None, None) == -2         # D % 4
    assert lib.hirest_cascade_trim_gather(p, None, p, p, 1, 1, 7, 8, 0, 20, p + 4, None, None) == -1     # misaligned
    assert lib.hirest_cascade_trim_gather(None, None, p, p, 1, 1, 7, 8, 0, 20, p, None, None) == -1
    assert lib.hirest_cascade_trim_gather(p, p, p, p, 1, 1, 7, 8, 4, 20, p, None, None) == -1            # asr without its output


# ------------------------------------------------------------------------------------------------------------ the model

class _Args:
    moment_segmentation_difference_threshold = 0.5
    moment_segmentation_max_iterations = 20
    max_frames_step_captioning = 20
    max_words = 48


@pytest.fixture(scope="module")
def model(dev, golden_dir):
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(golden_dir, "joint_schema.json"))).items()}
    sd = synth.joint_state_dict(shapes, 31)
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5
    m = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=_Args(), clip_model=None)
    assert not m.load_state_dict(sd, strict=False).missing_keys
    return m.to(dev).eval()


def _chain(model, batch, durations, n_frames, beams):
    """Three chained test_step calls, the chained batches built on the host by the dataset's rules (hirest_dataset.py:250-261,
    :285-304).  Zero-step samples are skipped in the captioning stage."""
    B, T = batch["vis_mask"].shape
    pred = model.test_step(dict(batch, tasks=["moment_retrieval"]))["prediction"]
    ts = [[frame_index_to_timestamp(f, durations[b], n_frames) for f in pred[b]] for b in range(B)]
    bf = [[timestamp_to_frame_index(t, durations[b], n_frames) for t in ts[b]] for b in range(B)]
    seg = model.test_step(dict(batch, tasks=["moment_segmentation"], moment_bound_frames=torch.tensor(bf)))["prediction"]
    step_ts, masks, rows = [], [], []
    for b in range(B):
        st, fr = ref.steps_of(seg[b], durations[b], n_frames)
        step_ts.append(st)
        for a, e in fr:
            masks.append(ref.caption_mask(a, e, T))
            rows.append(b)
    ids = []
    if rows:
        r = torch.tensor(rows)
        cap = {"tasks": ["step_captioning"], "vis_feats": batch["vis_feats"][r], "asr_feats": batch["asr_feats"][r],
               "moment_mask": torch.tensor(masks), "text_feat": batch["text_feat"][r]}
        ids = model.test_step(cap, num_beams=beams, return_ids=True)["token_ids"]
    caps, lo = [], 0
    for b in range(B):
        caps.append(ids[lo:lo + len(step_ts[b])])
        lo += len(step_ts[b])
    return {"moment_frames": pred, "bounds": ts, "boundary_frames": seg, "step_bounds": step_ts, "captions": caps}


def _synthetic_batch(name, B, T, durations):
    vis, asr, text, vis_mask, moment_mask, _ = synth.joint_inputs(name, B, T, 41)
    return {"vis_feats": vis, "asr_feats": asr, "text_feat": text, "vis_mask": torch.ones_like(vis_mask),
            "moment_mask": torch.ones_like(moment_mask), "video_duration": durations}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_end_to_end_equals_chained_test_steps(model, precision):
    B, T, durations = 3, 64, [64, 37, 130]
    model.set_precision(precision)
    try:
        found = 0
        for name in ("cascade.t0", "cascade.t1", "cascade.t2"):
            batch = dict(_synthetic_batch(name, B, T, durations), n_frames=T)
            got = model.end_to_end(batch, num_beams=5, return_ids=True)
            want = _chain(model, batch, durations, T, 5)
            assert got == want
            found += sum(len(s) for s in want["step_bounds"])
        assert found > 0                                                  # the captioning stage ran
    finally:
        model.set_precision("fp32")


def _golden_batch(golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "cascade_a.json")))
    g = np.load(os.path.join(golden_dir, "cascade_a.npz"))
    f32 = lambda k: torch.from_numpy((g[k].astype(np.uint32) << 16).view(np.float32).copy())
    B, T = gold["B"], gold["T"]
    batch = {"vis_feats": f32("vis_bf16"), "asr_feats": f32("asr_bf16"), "text_feat": f32("text_bf16"),
             "vis_mask": torch.ones((B, T), dtype=torch.long), "moment_mask": torch.ones((B, T), dtype=torch.long),
             "video_duration": g["durations"].tolist(), "n_frames": gold["n_model_frames"]}
    return gold, batch


@pytest.mark.parametrize("beams", [3, 5])
def test_end_to_end_equals_the_reference_chain(model, golden_dir, beams):
    gold, batch = _golden_batch(golden_dir)
    out = model.end_to_end(batch, num_beams=beams, return_ids=True)
    assert out["moment_frames"] == gold["moment_frames"] and out["bounds"] == gold["bounds"]
    assert out["boundary_frames"] == gold["boundary_frames"] and out["step_bounds"] == gold["step_bounds"]
    assert [c for caps in out["captions"] for c in caps] == gold["token_ids"][str(beams)]
    final = cascade.end_to_end_results(gold["split"], gold["prompts"], gold["video_fnames"], out)
    assert final == gold["final"][str(beams)]
    # strings (the default) give the same dict
    out_s = model.end_to_end(batch, num_beams=beams)
    assert cascade.end_to_end_results(gold["split"], gold["prompts"], gold["video_fnames"], out_s) == gold["final"][str(beams)]


def test_run_end_to_end_over_two_batches(model, golden_dir):
    gold, b0 = _golden_batch(golden_dir)
    b1 = dict(_synthetic_batch("cascade.t0", 3, 64, [64, 37, 130]), n_frames=64)
    both = cascade.run_end_to_end(model, [b0, b1], num_beams=5, return_ids=True)
    alone = [model.end_to_end(b0, num_beams=5, return_ids=True), model.end_to_end(b1, num_beams=5, return_ids=True)]
    assert both == alone
    # a cap that forces one search per batch gives the same result
    assert cascade.run_end_to_end(model, [b0, b1], num_beams=5, return_ids=True, rows_in_flight=5) == alone
    assert hirest_amd.run_end_to_end is cascade.run_end_to_end and hirest_amd.end_to_end_results is cascade.end_to_end_results
