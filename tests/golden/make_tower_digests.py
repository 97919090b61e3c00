"""SHA-256 of what the EVA-CLIP and OpenAI-CLIP towers return at every precision, split rule and input type, over the public
surface only (build_eva_model_and_transforms, clip.build_model, set_precision, encode_image / encode_text and the
max_*_per_call attributes), so the same script runs before and after a change to the Python that prepares weights and
issues the tower calls.  tests/golden/tower_digests.json is its output at the commit named inside the file;
tests/test_gpu_tower_digests.py recomputes the digests and asserts they are equal.

Needs an MI355X.  Run at the commit whose bits are to be pinned:

    python tests/golden/make_tower_digests.py --commit $(git rev-parse HEAD)
"""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SEED = 23


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def eva_model(dev):
    import hirest_amd
    model, _ = hirest_amd.build_eva_model_and_transforms("EVA_CLIP_tiny_test", pretrained=f"synth:{SEED}", precision="bf16")
    return model.to(dev).eval()


def openai_model(dev):
    from hirest_amd import clip, synth
    return clip.build_model(synth.openai_clip_state_dict(synth.OPENAI_VIT_TINY, SEED)).to(dev)


def eva_inputs(dev):
    from hirest_amd import synth
    return {"img": synth.frames("towerdig.img", (130, 3, 224, 224), SEED + 1).to(dev),
            "u8": torch.from_numpy(synth.rgb_frames("towerdig.u8", (3, 224, 224, 3), SEED + 2)).to(dev),
            "tok": synth.tokens("towerdig.tok", 5, SEED + 3).to(dev)}


def eva_case(model, inp, precision, what, n, **limits):
    """One encode at ``precision`` with the per-call limits in ``limits`` set for this call only."""
    tower = model.text if what == "tok" else model.visual
    old = {k: getattr(tower, k) for k in limits}
    model.set_precision(precision)
    for k, v in limits.items():
        setattr(tower, k, v)
    try:
        return (model.encode_text if what == "tok" else model.encode_image)(inp[what][:n])
    finally:
        for k, v in old.items():
            setattr(tower, k, v)


# name -> (precision, input, rows, per-call limits): the smallest shapes that reach every branch of the call loops
EVA_CASES = {
    "eva.bf16.3": ("bf16", "img", 3, {}),                                                # unfolded LayerNorm
    "eva.bf16.64": ("bf16", "img", 64, {}),                                              # folded
    "eva.bf16.130.max70": ("bf16", "img", 130, {"max_frames_per_call": 70}),             # 65 + 65, folded
    "eva.bf16.130.max48": ("bf16", "img", 130, {"max_frames_per_call": 48}),             # 44 + 44 + 42, unfolded
    "eva.fp32.5.max2": ("fp32", "img", 5, {"max_frames_per_call_f32": 2}),               # 2 + 2 + 1
    "eva.bf16x3.5": ("bf16x3", "img", 5, {}),
    "eva.bf16x3.70.max40": ("bf16x3", "img", 70, {"max_frames_per_call_x3": 40}),        # 35 + 35
    "eva.text.bf16.5.max2": ("bf16", "tok", 5, {"max_rows_per_call": 2}),
    "eva.text.fp32.5.max2": ("fp32", "tok", 5, {"max_rows_per_call": 2}),
    "eva.bf16.u8": ("bf16", "u8", 3, {}),
    "eva.fp32.u8": ("fp32", "u8", 3, {}),
}


def eva_digests(model, inp):
    out, fallbacks = {}, model.visual.fold_fallbacks
    for name, (precision, what, n, limits) in EVA_CASES.items():
        out[name] = digest(eva_case(model, inp, precision, what, n, **limits))
        if precision == "bf16" and what != "tok":
            out[name + ".last_fold_ratio"] = float(model.visual.last_fold_ratio).hex()
    out["eva.fold_fallbacks"] = int(model.visual.fold_fallbacks - fallbacks)
    return out


def openai_digests(model, dev):
    from hirest_amd import synth
    img = synth.frames("towerdig.oa.img", (3, 3, 224, 224), SEED + 4).to(dev)
    tok = synth.tokens("towerdig.oa.tok", 3, SEED + 5).to(dev)
    out = {}
    for precision in ("bf16", "fp32"):
        model.set_precision(precision)
        for pip_head in (False, True):
            model.visual.pip_head = pip_head
            out[f"openai.{precision}.3." + ("cls" if pip_head else "patches")] = digest(model.encode_image(img))
        model.visual.pip_head = False
        out[f"openai.text.{precision}.3"] = digest(model.encode_text(tok))
    return out


def all_digests(dev):
    out = eva_digests(eva_model(dev), eva_inputs(dev))
    out.update(openai_digests(openai_model(dev), dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit this runs at (recorded in the file)")
    ap.add_argument("--out", default=os.path.join(HERE, "tower_digests.json"))
    a = ap.parse_args()
    res = {"commit": a.commit, "seed": SEED, "digests": all_digests(torch.device("cuda:0"))}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
