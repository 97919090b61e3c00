"""CLIPScore on the device: the hirest_clip_score kernel against fp64 torch, the whole pipeline (decode, preprocess, CLS head, text
tower, kernel) against the real reference's recorded run (tests/golden/clipscore.*), and the pip head against transformers."""
import json
import os

import numpy as np
import pytest
import torch

from hirest_amd import evaluation, ops, synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "clipscore.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def frame_dir(tmp_path_factory):
    from test_clip_score_host import write_frames
    return write_frames(tmp_path_factory.mktemp("clipscore_gpu"))


def _model(dev, golden, tmp_path_factory, precision):
    from hirest_amd import clip
    path = os.path.join(str(tmp_path_factory.mktemp("ckpt")), "tiny.pt")
    torch.save(synth.openai_clip_state_dict(synth.OPENAI_VIT_TINY, golden["seed"]), path)
    model, _ = clip.load(path, device=dev, pip_head=True, precision=precision)
    return model


def _ref_scores(img, txt, sel):
    i = img.double().cpu()
    t = txt.double().cpu()
    i = i / i.norm(dim=1, keepdim=True)
    t = t / t.norm(dim=1, keepdim=True)
    return (i[sel.long()] * t[:, None, :]).sum(-1).mean(-1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E", [64, 512, 768, 1024])
def test_kernel_against_fp64(dev, dtype, E):
    g = torch.Generator().manual_seed(E)
    U = 501
    img = torch.randn(U, E, generator=g).to(dtype)
    for C in (1, 7, 3856):
        txt = torch.randn(C, E, generator=g).to(dtype)
        for K in (1, 4):
            sel = torch.randint(0, U, (C, K), generator=g, dtype=torch.int32)
            if K == 4 and C > 1:
                sel[0] = torch.tensor([5, 5, 5, 2])                   # repeated and out-of-order ids
                sel[1] = torch.tensor([U - 1, 0, U - 1, 3])
            got = ops.clip_score(img.to(dev), txt.to(dev), sel).cpu()
            ref = _ref_scores(img, txt, sel)                          # fp64 of the same (bf16-rounded) values
            err = (got.double() - ref).abs().max().item()
            assert err <= 1e-6, (dtype, E, C, K, err)


def test_kernel_batch_invariance(dev):
    g = torch.Generator().manual_seed(3)
    U, C, E, K = 900, 3856, 512, 4
    img = torch.randn(U, E, generator=g).to(dev)
    txt = torch.randn(C, E, generator=g).to(dev)
    sel = torch.randint(0, U, (C, K), generator=g, dtype=torch.int32)
    full = ops.clip_score(img, txt, sel)
    for c in (0, 1, 1234, C - 1):
        one = ops.clip_score(img, txt[c:c + 1].contiguous(), sel[c:c + 1])
        assert torch.equal(one, full[c:c + 1]), c
    mixed = ops.clip_score(img, txt.to(torch.bfloat16), sel)          # mixed operand dtypes take their own instantiation
    assert (mixed - full).abs().max().item() < 1e-2
    with pytest.raises(RuntimeError):
        ops.clip_score(img, txt, torch.full((C, K), U, dtype=torch.int32))


def _run(model, golden, frame_dir, monkeypatch):
    from hirest_amd import jpeg
    decoded = []
    orig = jpeg.Decoder.decode

    def counting(self, sources, device=None):
        decoded.extend(bytes(s) for s in sources)
        return orig(self, sources, device)
    monkeypatch.setattr(jpeg.Decoder, "decode", counting)
    per = evaluation.caption_clip_scores(golden["gt"], golden["pred"], model, frame_dir)
    res = {k: evaluation.evaluate_clip_score(golden["gt"], golden["pred"], golden["video_to_cat"], model, frame_dir, per_category=pc)
           for k, pc in (("all", False), ("per_category", True))}
    return per, res, decoded, list(jpeg.last_fallbacks)


def _check(per, res, golden, frame_dir, per_bar, cat_bar):
    from hirest_amd import jpeg  # noqa: F401
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir)
    want = [c["score"] for c in golden["runs"]["all"]["calls"]]
    got = [s for _, _, s in per if s is not None]
    assert [s is None for _, _, s in per] == plan.skip
    assert len(got) == len(want)
    err = max(abs(a - b) for a, b in zip(got, want))
    cat_err = 0.0
    for run in ("all", "per_category"):
        ref = golden["runs"][run]["result"]
        assert set(res[run]) == set(ref)
        for c in ref:
            assert res[run][c]["Total"] == ref[c]["Total"]
            cat_err = max(cat_err, abs(res[run][c]["CLIPScore"] - ref[c]["CLIPScore"]))
    print(f"per-caption max |diff| {err:.3e}, per-category CLIPScore max |diff| {cat_err:.3e}")
    assert err <= per_bar and cat_err <= cat_bar, (err, cat_err)


def test_end_to_end_fp32_matches_reference(dev, golden, frame_dir, tmp_path_factory, monkeypatch):
    model = _model(dev, golden, tmp_path_factory, "fp32")
    per, res, decoded, fallbacks = _run(model, golden, frame_dir, monkeypatch)
    _check(per, res, golden, frame_dir, 2e-5, 1e-5)
    plan = evaluation.clip_score_plan(golden["gt"], golden["pred"], frame_dir)
    # each unique frame decoded once per evaluation call (three calls above)
    assert len(decoded) == 3 * len(plan.frames)
    assert len(set(decoded)) == len(plan.frames)
    # the last call's host-decoded files are exactly the ones the fixture marks (its progressive frame)
    names = [os.path.relpath(plan.frames[i], frame_dir) for i, _ in fallbacks]
    assert names == golden["fallbacks"]


def test_end_to_end_bf16_towers(dev, golden, frame_dir, tmp_path_factory, monkeypatch):
    """The default bf16 towers.  Measured on the fixture: 1.2e-3 per caption, 5.8e-4 per category; the bars leave 2.5x of that
    (the fp32 run above is the one to report)."""
    model = _model(dev, golden, tmp_path_factory, "bf16")
    per, res, _, _ = _run(model, golden, frame_dir, monkeypatch)
    _check(per, res, golden, frame_dir, 3e-3, 1.5e-3)


def test_pip_head_matches_transformers(dev, golden, tmp_path_factory):
    """fp32 CLS image embedding and text embedding against transformers' CLIPModel on the same weights (make_clipscore_golden.py)."""
    model = _model(dev, golden, tmp_path_factory, "fp32")
    g = np.load(os.path.join(GOLDEN, "clipscore.npz"))
    img = synth.frames(golden["hf_image_frames"], (4, 3, 224, 224), golden["hf_image_seed"])
    got_i = model.encode_image(img.to(dev)).cpu()
    got_t = model.encode_text(torch.from_numpy(g["hf_tokens"]).to(dev)).cpu()
    for got, ref, what in ((got_i, g["hf_image_features"], "image"), (got_t, g["hf_text_features"], "text")):
        ref = torch.from_numpy(ref)
        cos = torch.nn.functional.cosine_similarity(got, ref).min().item()
        rel = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
        print(f"{what}: min cos {cos:.9f}, max rel err {rel:.2e}")
        assert cos >= 1 - 1e-6 and rel <= 1e-5, (what, cos, rel)
