"""The towers return the bits they returned at the commit recorded in tests/golden/tower_digests.json: every precision, both split
rules of the micro-batch loop, the folded and the unfolded LayerNorm path, float and uint8 frames, both CLIP heads
(tests/golden/make_tower_digests.py lists the cases and computes the digests; this file only compares).  And the weight
preparations of the three precisions live side by side: switching precision back and forth neither changes a result nor rebuilds
what was built."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_tower_digests as mk  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want(golden_dir):
    return json.load(open(os.path.join(golden_dir, "tower_digests.json")))["digests"]


@pytest.fixture(scope="module")
def eva(dev):
    return mk.eva_model(dev), mk.eva_inputs(dev)


def _assert_same(got, want, prefix):
    want = {k: v for k, v in want.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want)
    assert got == want, "changed: " + ", ".join(k for k in got if got[k] != want[k])


def test_eva_towers_bit_identical(eva, want):
    _assert_same(mk.eva_digests(*eva), want, "eva.")


def test_openai_towers_bit_identical(dev, want):
    _assert_same(mk.openai_digests(mk.openai_model(dev), dev), want, "openai.")


def test_precisions_keep_their_preparations(eva, want):
    model, inp = eva
    model.visual._prepared = None
    first, bf16_prep = {}, None
    for precision in ("bf16", "bf16x3", "bf16", "fp32", "bf16"):
        got = mk.digest(mk.eva_case(model, inp, precision, "img", 5))
        assert first.setdefault(precision, got) == got, f"{precision} changed after a switch of precision"
        if bf16_prep is None:
            bf16_prep = model.visual._prepared["bf16"]
    assert first["bf16x3"] == want["eva.bf16x3.5"]
    assert model.visual._prepared["bf16"] is bf16_prep                      # nothing was evicted ...
    assert set(model.visual._prepared) == {"bf16", "fp32", "x3"}            # ... and every kind is resident
    model.visual._prepared = None                                           # an outside reset drops all of them
    assert mk.digest(mk.eva_case(model, inp, "bf16", "img", 5)) == first["bf16"]
    assert set(model.visual._prepared) == {"bf16"}
