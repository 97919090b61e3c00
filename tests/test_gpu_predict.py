"""hirest_amd.predict on the GPU against the dicts the REAL reference's ``Trainer.predict`` returned for the same two-batch loaders
(tests/golden/valid_predict.json, made by make_valid_golden.py): keys, order and values exact, the loss within the bars of
tests/test_gpu_valid.py."""
import json
import os

import pytest
import torch

from hirest_amd import synth

pytestmark = pytest.mark.gpu

LOSS_BAR = {"fp32": 1e-5, "bf16x3": 2e-4}


class Loader(list):
    def __init__(self, batches, task):
        super().__init__(batches)
        self.task = task


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
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5
    m = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=None, clip_model=None)
    m.load_state_dict(sd, strict=False)
    return m.to(dev).eval()


def _loader(task):
    return Loader([synth.valid_batches(c)[task] for c in synth.TRAIN_CASES], task)


def _same(got, want):
    """Equal values AND equal key order, all the way down."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (list(got), list(want))
        for k in want:
            _same(got[k], want[k])
    else:
        assert got == want, (got, want)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("key", ["moment_retrieval.target.beam5", "moment_segmentation.plain.beam5", "moment_segmentation.target.beam5",
                                 "step_captioning.target.beam5", "step_captioning.plain.beam3"])
def test_predict_equals_the_reference_dicts(model, golden_dir, key, precision):
    import hirest_amd
    want = json.load(open(os.path.join(golden_dir, "valid_predict.json")))[key]
    task, mode, beams = key.split(".")
    has_target = mode == "target"
    model.set_precision(precision)
    try:
        got = hirest_amd.predict(model, _loader(task), has_target=has_target, num_beams=int(beams[4:]), n_model_frames=-1)
    finally:
        model.set_precision("fp32")
    assert ("loss" in got) == has_target == ("loss" in want)
    if has_target:
        dev_l = abs(float(got["loss"]) - want["loss"]) / abs(want["loss"])
        print(f"[{precision}] {key}: loss {float(got['loss']):.7f} (reference {want['loss']:.7f}), relative deviation {dev_l:.2e}")
        assert dev_l <= LOSS_BAR[precision]
        assert list(got)[-1] == "loss"
        got, want = {k: v for k, v in got.items() if k != "loss"}, {k: v for k, v in want.items() if k != "loss"}
    _same(got, want)


def test_predict_captioning_without_targets_is_per_batch_test_step(model):
    import hirest_amd
    loader = _loader("step_captioning")
    got = hirest_amd.predict(model, loader, has_target=False, num_beams=5)
    want = {}
    for b in loader:
        for video, dur, sentence in zip(b["video_fnames"], b["video_duration"], model.test_step(b, num_beams=5)["prediction"]):
            e = want.setdefault(video, {})
            e.setdefault("captions", []).append({"sentence": sentence})
            e["video_duration"] = dur
    _same(got, want)
