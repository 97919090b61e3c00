"""The validation pass on the GPU: MomentModel.valid_step (loss and prediction from one forward) against the REAL reference's
``train_step`` loss in eval mode and ``test_step`` prediction (tests/golden/valid_steps.json, made by make_valid_golden.py), and its
two kernels (csrc/valid.hip) against fp64 torch on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from hirest_amd import synth

pytestmark = pytest.mark.gpu

LOSS_BAR = {"fp32": 1e-5, "bf16x3": 2e-4}          # relative, as tests/test_gpu_train.py holds the same quantities


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, golden_dir):
    import hirest_amd
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(golden_dir, "joint_schema.json"))).items()}
    sd = synth.joint_state_dict(shapes, 31)
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5        # the fixtures' model (gen_caption's raise)
    m = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=None, clip_model=None)
    m.load_state_dict(sd, strict=False)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "valid_steps.json")))


@pytest.fixture(scope="module")
def batches():
    return {case: synth.valid_batches(case) for case in synth.TRAIN_CASES}


def _first(batch, n):
    """The first n samples of a loader batch."""
    B = len(batch["tasks"])
    return {k: (v[:n] if (torch.is_tensor(v) or isinstance(v, list)) and len(v) == B else v) for k, v in batch.items()}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_valid_step_vs_reference(model, golden, batches, case, precision):
    """Measured (MI355X): see DESIGN 4.14 — the printed deviations are the ones quoted there."""
    model.set_precision(precision)
    g, bar = golden[case], LOSS_BAR[precision]
    res = model.valid_step(batches[case]["moment_retrieval"])
    dev_r = abs(res["loss"].item() - g["retrieval_loss"]) / abs(g["retrieval_loss"])
    print(f"[{precision}] case {case}: retrieval loss {res['loss'].item():.7f} (reference {g['retrieval_loss']:.7f}), relative deviation {dev_r:.2e}")
    assert res["loss"].dim() == 0 and res["loss"].dtype == torch.float32 and res["loss"].is_cuda and not res["loss"].requires_grad
    assert res["prediction"] == g["retrieval_prediction"]
    assert dev_r <= bar
    assert g["argmax_margin"] > 2e-3                # why index-exact is a fair demand at bf16x3 (the encoder's logit bar)
    for beams in (3, 5):
        cap = model.valid_step(batches[case]["step_captioning"], num_beams=beams, return_ids=True)
        dev_c = abs(cap["loss"].item() - g["caption_loss"]) / abs(g["caption_loss"])
        print(f"[{precision}] case {case}: captioning loss {cap['loss'].item():.7f} (reference {g['caption_loss']:.7f}), relative deviation {dev_c:.2e}")
        assert cap["prediction"] == g[f"caption_prediction_beam{beams}"]
        assert [" ".join(str(i) for i in h) for h in cap["token_ids"]] == g[f"caption_prediction_beam{beams}"]
        assert cap["loss"].dim() == 0 and dev_c <= bar
    model.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_valid_step_prediction_is_test_steps(model, batches, precision):
    model.set_precision(precision)
    for case in ("a", "b"):
        for task, kw in (("moment_retrieval", {}), ("moment_segmentation", {}), ("step_captioning", {"num_beams": 3, "return_ids": True})):
            b = batches[case][task]
            got, want = model.valid_step(b, **kw), model.test_step(b, **kw)
            assert "loss" in got and {k: v for k, v in got.items() if k != "loss"} == want, (case, task)
    # moment segmentation: with targets train_step's loss (eval mode) beside the prediction, without them test_step's result alone
    seg = batches["a"]["moment_segmentation"]
    with torch.no_grad():
        want = model.train_step(seg)["loss"].item()
    assert abs(model.valid_step(seg)["loss"].item() - want) <= 1e-6 * abs(want)
    bare = {k: v for k, v in seg.items() if k not in ("prev_boundary_mask", "moment_segmentation_target")}
    assert model.valid_step(bare) == model.test_step(bare) and "loss" not in model.valid_step(bare)
    with pytest.raises(NotImplementedError):
        model.valid_step({"tasks": ["something_else"]})
    model.set_precision("fp32")


def test_valid_step_repeats_bit_for_bit_and_ignores_training_mode(model, batches):
    for task, kw in (("moment_retrieval", {}), ("step_captioning", {"num_beams": 3})):
        b = batches["a"][task]
        first = model.valid_step(b, **kw)
        for _ in range(2):
            again = model.valid_step(b, **kw)
            assert torch.equal(again["loss"], first["loss"]) and again["prediction"] == first["prediction"]
        model.train()                                # dropout stays off: the loss is the eval-mode loss whatever the mode
        try:
            assert torch.equal(model.valid_step(b, **kw)["loss"], first["loss"])
        finally:
            model.eval()


def test_valid_step_batch_invariance(model, batches):
    for task, kw in (("moment_retrieval", {}), ("step_captioning", {"num_beams": 5})):
        b = batches["a"][task]
        assert model.valid_step(_first(b, 1), **kw)["prediction"][0] == model.valid_step(b, **kw)["prediction"][0]


def test_non_prefix_decoder_mask_takes_the_training_forward(model, batches):
    """A padded key IN FRONT of a target position: the causal penalty alone is not the reference's mask, so the loss comes from
    train_step's forward (which applies both).  Equal up to the order of train_step's atomic row sums (a few ulp)."""
    b = dict(batches["a"]["step_captioning"])
    tt = [list(t) for t in b["target_text"]]
    tt[0][6] = list(tt[0][6])
    tt[0][6][2] = 0
    b["target_text"] = [tuple(t) for t in tt]
    inp, mask, out = model._caption_targets(b)
    assert not model._causal_mask_is_exact(mask, out) and model._causal_mask_is_exact(*model._caption_targets(batches["a"]["step_captioning"])[1:])
    with torch.no_grad():
        want = model.train_step(b)["loss"].item()
    got = model.valid_step(b, num_beams=3)
    assert abs(got["loss"].item() - want) <= 1e-6 * abs(want)
    plain = model.valid_step(batches["a"]["step_captioning"], num_beams=3)
    assert got["prediction"] == plain["prediction"] and got["loss"].item() != plain["loss"].item()      # the mask does matter
    # no target at all: what train_step returns for an all-ignored batch
    none = dict(b, target_text=[tuple(list(t[:7]) + [[-1] * len(t[7])] + [t[8]]) for t in batches["a"]["step_captioning"]["target_text"]])
    with torch.no_grad():
        want0 = model.train_step(none)["loss"]
    got0 = model.valid_step(none, num_beams=3)["loss"]
    assert got0.dim() == 0 and got0.item() == want0.item() == 0.0


def test_caption_loss_leg_never_stores_the_logits(model, dev):
    """Derived from sizes: B = 4 captions with a target at all 48 positions are R = 192 rows; their logits would be R * Vp * 4 bytes
    (23 MB).  After a warm-up call the loss leg's peak allocation stays below that."""
    B, L = 4, 48
    vis, asr, text, vis_mask, _, _ = synth.joint_inputs("valid.mem", B, 64, 59)
    mm = torch.zeros(B, 64, dtype=torch.long)
    mm[:, 5:25] = 1
    batch = {"tasks": ["step_captioning"] * B, "vis_feats": vis, "vis_mask": vis_mask, "moment_mask": mm, "asr_feats": asr, "text_feat": text}
    u = ((synth.uniform_pm1("valid.mem.words", B * L, 59).reshape(B, L) + 1.0) * 0.5 * 29000).astype(np.int64) + 1000
    inp = np.concatenate([np.full((B, 1), 101, dtype=np.int64), u[:, :L - 1]], 1)
    out = np.concatenate([u[:, :L - 1], np.full((B, 1), 102, dtype=np.int64)], 1)
    with torch.no_grad():
        enc_kv = model._caption_encoder_kv(*model._caption_inputs(batch, dev))
        first = model._caption_loss(enc_kv, inp, out)                    # warm-up: workspaces, kernel configuration
        torch.cuda.synchronize()
        level = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        loss = model._caption_loss(enc_kv, inp, out)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - level
    Vp = model._w()["lm_w"].shape[0]
    print(f"loss leg at R = {B * L}: peak {peak / 2**20:.1f} MiB above the level before it; the logits would be {B * L * Vp * 4 / 2**20:.1f} MiB")
    assert torch.equal(loss, first) and torch.isfinite(loss)
    assert peak < B * L * Vp * 4


# ------------------------------------------------------------------------------------------------ hirest_moment_valid_f32

def _moment_case(B, T, variant, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(2, B, T, generator=g) * 3.0
    lens = torch.randint(1, T + 1, (B,), generator=g)
    vis = (torch.arange(T)[None, :] < lens[:, None]).to(torch.int32)
    mm = (torch.rand(B, T, generator=g) < 0.6).to(torch.int32) * vis
    st, et = torch.randint(0, T, (B,), generator=g).to(torch.int32), torch.randint(0, T, (B,), generator=g).to(torch.int32)
    st[0], et[0] = 0, T - 1                                              # targets at both ends
    st[B - 1], et[B - 1] = T - 1, 0
    if variant == "zero_vis":
        vis[0] = 0                                                       # every frame holds the fill: index 0
    elif variant == "zero_moment":
        mm[:] = 0                                                        # the clamp: 0 / max(0, 1)
    elif variant == "tie" and T > 2:
        vis[B - 1] = 1
        i, j = T // 3, T - 1
        logits[:, B - 1, i] = logits[:, B - 1, j] = logits[:, B - 1].max() + 1.0       # an exact tie: the first index
    return logits.reshape(2, B * T).contiguous(), vis.contiguous(), mm.contiguous(), st, et


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T", [1, 65, 2048])
def test_moment_valid_kernel_vs_fp64(dev, B, T):
    from hirest_amd import _lib, ops
    lib = _lib.load()
    for variant in ("plain", "zero_vis", "zero_moment", "tie"):
        logits, vis, mm, st, et = _moment_case(B, T, variant, 1000 * B + T)
        x = logits.reshape(2, B, T)
        want_idx = torch.stack([torch.where(vis == 1, x[h], torch.tensor(-1e10)).argmax(dim=1) for h in range(2)], dim=1)
        x64, m64 = x.double(), mm.double()
        hot = [torch.zeros(B, T, dtype=torch.float64).scatter_(1, t.long().unsqueeze(1), 1.0) for t in (st, et)]
        per = [torch.nn.functional.binary_cross_entropy_with_logits(x64[h], hot[h], reduction="none") * m64 for h in range(2)]
        ref = float((per[0].sum() / m64.sum().clamp(min=1) + per[1].sum() / m64.sum().clamp(min=1)) / 2)
        d = [t.to(dev) for t in (logits, vis, mm, st, et)]
        pred, loss = ops.moment_valid(*d)
        # the existing pair on the same inputs: two hirest_bce_masked_f32 launches adding 0.5 * BCE each, as the training step calls them
        acc = torch.zeros(1, dtype=torch.float32, device=dev)
        dl = torch.empty(B * T, dtype=torch.float32, device=dev)
        for h, tg in enumerate((d[3], d[4])):
            _lib.check(lib.hirest_bce_masked_f32(d[0][h].data_ptr(), tg.data_ptr(), d[2].data_ptr(), B, T, 0.5, acc.data_ptr(), dl.data_ptr(),
                                                 ops.stream_ptr()), "bce_masked")
        err, err_pair = abs(float(loss.item()) - ref), abs(float(acc.item()) - ref)
        print(f"B {B} T {T} {variant}: loss {loss.item():.7f} fp64 {ref:.9f} error {err:.2e} (existing pair {err_pair:.2e})")
        assert pred.cpu().tolist() == want_idx.tolist(), variant
        if variant == "zero_vis":
            assert pred[0].tolist() == [0, 0]
        if variant == "tie" and T > 2:
            assert pred[B - 1].tolist() == [T // 3, T // 3]
        if variant == "zero_moment":
            assert loss.item() == 0.0
        assert err <= 2 * err_pair, variant
        again = ops.moment_valid(*d)
        assert torch.equal(again[0], pred) and torch.equal(again[1], loss)
        if B > 1:                                                        # a sample's indices are its own
            one = ops.moment_valid(d[0].reshape(2, B, T)[:, 5:6].reshape(2, T).contiguous(), d[1][5:6], d[2][5:6], d[3][5:6], d[4][5:6])
            assert one[0][0].tolist() == pred[5].tolist()


# ------------------------------------------------------------------------------------------------ hirest_lm_head_ce_f32

def _head_inputs(V, scale, seed):
    """200 rows against a V-column head padded as the weight cache pads it (rows to a multiple of 4, zero weights, bias -3e38), and
    the fp64 nll of every row, computed once per (V, scale)."""
    g = torch.Generator().manual_seed(seed)
    R, K = 200, 768
    h = torch.randn(R, K, generator=g)
    w = torch.randn(V, K, generator=g) * scale
    b = torch.randn(V, generator=g)
    tgt = torch.randint(0, V, (R,), generator=g).to(torch.int32)
    tgt[0], tgt[1] = 0, V - 1                                            # first and last real column
    tgt[2] = tgt[3]                                                      # rows that share a target
    pad = (-V) % 4
    wp = torch.cat([w, torch.zeros(pad, K)]).contiguous()
    bp = torch.cat([b, torch.full((pad,), -3.0e38)]).contiguous()
    logits = h.double() @ w.double().t() + b.double()
    ref = torch.logsumexp(logits, dim=1) - logits.gather(1, tgt.long().unsqueeze(1)).squeeze(1)
    return h, wp, bp, tgt, ref, float(logits.abs().max())


_HEAD_CACHE = {}


def _head(V, scale, dev):
    key = (V, scale)
    if key not in _HEAD_CACHE:
        h, wp, bp, tgt, ref, top = _head_inputs(V, scale, 7 + V)
        _HEAD_CACHE[key] = ([t.to(dev) for t in (h, wp, bp, tgt)], ref.numpy(), top)
    return _HEAD_CACHE[key]


@pytest.mark.parametrize("V,scale", [(17, 0.05), (1000, 0.05), (30522, 0.05), (30522, 0.75)])
def test_lm_head_ce_kernel_vs_fp64(dev, V, scale):
    """(30522, 0.75): logits of magnitude ~80 — the running maximum has to carry the sum."""
    import hirest_amd
    from hirest_amd import _lib, ops
    lib = _lib.load()
    (h, wp, bp, tgt), ref, top = _head(V, scale, dev)
    Vp = wp.shape[0]
    # the existing pair on the same inputs: hirest_gemm_f32 writes the logits, hirest_ce_rows_f32 reduces one row per call
    logits = hirest_amd.MomentModel._gemm(h, wp, bp)
    dl = torch.empty(Vp, dtype=torch.float32, device=dev)
    pair = torch.zeros(200, dtype=torch.float32, device=dev)
    for r in range(200):
        _lib.check(lib.hirest_ce_rows_f32(logits[r].data_ptr(), Vp, tgt[r:r + 1].data_ptr(), 1, Vp, 1.0, 1, pair[r:r + 1].data_ptr(), dl.data_ptr(),
                                          ops.stream_ptr()), "ce_rows")
    err_pair = np.abs(pair.cpu().numpy().astype(np.float64) - ref)
    full = None
    for R in (200, 33, 1):
        nll, loss = ops.lm_head_ce(h[:R], wp, bp, tgt[:R])
        got = nll.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.isfinite(loss.item())       # the -3e38 pad columns leave no inf or NaN
        err = np.abs(got - ref[:R])
        bar = np.maximum(2 * err_pair[:R].max(), np.spacing(np.abs(ref[:R]).astype(np.float32)).astype(np.float64))
        print(f"V {V} (|logit| up to {top:.0f}) R {R}: worst nll error {err.max():.2e}, existing gemm + ce_rows {err_pair[:R].max():.2e}")
        assert (err <= bar).all(), (R, err.max(), err_pair[:R].max())
        assert abs(loss.item() - ref[:R].mean()) <= 2e-6 * abs(ref[:R].mean())
        if full is None:
            full = nll
        assert torch.equal(nll, full[:R])                                # a row's bits do not depend on how many rows there are
        assert torch.equal(ops.lm_head_ce(h[:R], wp, bp, tgt[:R])[0], nll)
    alone = ops.lm_head_ce(h[137:138].contiguous(), wp, bp, tgt[137:138].contiguous())[0]
    assert torch.equal(alone, full[137:138])
    # ignored rows: nll 0, the mean over the others
    t2 = tgt[:33].clone()
    t2[::2] = -1
    nll2, loss2 = ops.lm_head_ce(h[:33], wp, bp, t2, n_valid=16)
    assert torch.equal(nll2[1::2], full[1:33:2]) and float(nll2[::2].abs().max()) == 0.0
    assert abs(loss2.item() - ref[1:33:2].mean()) <= 2e-6 * abs(ref[1:33:2].mean())


def test_lm_head_ce_argument_errors(dev):
    from hirest_amd import _lib, ops
    lib = _lib.load()
    h, w, b = torch.zeros(4, 768, device=dev), torch.zeros(20, 768, device=dev), torch.zeros(20, device=dev)
    t = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.lm_head_ce(h, w[:, :764], b, t)
    with pytest.raises(ValueError):
        ops.lm_head_ce(h, w, b[:19], t)
    with pytest.raises(ValueError):
        ops.lm_head_ce(h, w, b, t, n_valid=5)
    with pytest.raises(RuntimeError):
        ops.lm_head_ce(h, w, b, t.long())
    with pytest.raises(RuntimeError, match="HIREST_E_SHAPE"):
        ops.lm_head_ce(h[:, :512].contiguous(), w[:, :512].contiguous(), b, t)
    with pytest.raises(ValueError):
        ops.moment_valid(torch.zeros(2, 10, device=dev), torch.zeros(2, 6, dtype=torch.int32, device=dev),
                         torch.zeros(2, 6, dtype=torch.int32, device=dev), t[:2], t[:2])
    assert lib.hirest_lm_head_ce_f32(h.data_ptr(), 768, w.data_ptr(), 768, b.data_ptr(), t.data_ptr(), 4, 20, 768, 4, h.data_ptr(), h.data_ptr(),
                                     h.data_ptr(), 8, None) == -3      # workspace too small: nothing launched
