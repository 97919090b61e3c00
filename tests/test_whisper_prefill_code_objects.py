"""Register allocation of the ragged prefill kernels, read from the gfx950 code object as
tests/test_whisper_align_code_objects.py reads the alignment's: whisper_prefill.o holds exactly these kernels, and none of them has
spilled registers or scratch.  The attention kernels of joint.o, whose body the ragged forms share (csrc/attention_f32.h), keep their
names and stay free of both as well."""
import os

import pytest

from test_code_objects import LIB, kernel_notes

ATTENTION = tuple(f"attention_f32_ragged_{kind}_kernel<{nw}>" for kind in ("causal", "cross") for nw in (1, 3, 4))
KERNELS = ("prefill_embed_kernel", "prefill_scatter_kernel", "prefill_gather_kernel") + ATTENTION


def _short(name):
    """the kernel's name without return type, namespace and argument list"""
    return name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]


def _notes(obj, tmp_path):
    path = os.path.join(LIB, obj)
    if not os.path.isfile(path):
        pytest.skip(f"{obj} not built (run __graft_entry__.build())")
    return {_short(k): v for k, v in kernel_notes(path, str(tmp_path)).items()}


def test_prefill_kernels_do_not_spill(tmp_path):
    notes = _notes("whisper_prefill.o", tmp_path)
    assert sorted(notes) == sorted(KERNELS), sorted(notes)
    for k in KERNELS:
        v = notes[k]
        print(k, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


def test_shared_body_left_the_attention_kernels_of_joint_as_they_were(tmp_path):
    notes = _notes("joint.o", tmp_path)
    names = [f"attention_f32_kernel<{dhp}, {nw}>" for dhp in (32, 64, 96) for nw in (1, 3, 4)]
    for k in names:
        assert k in notes, (k, sorted(n for n in notes if "attention_f32" in n))
    for nw in (1, 3, 4):            # the 64-wide heads of the decoder: no spills, no scratch
        v = notes[f"attention_f32_kernel<64, {nw}>"]
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (nw, v)
    for nw in (1, 3, 4):            # the same body, the same registers: a ragged form allocates what the packed form of its shape does
        a, b = notes[f"attention_f32_kernel<64, {nw}>"], _notes("whisper_prefill.o", tmp_path)[f"attention_f32_ragged_causal_kernel<{nw}>"]
        assert abs(a["vgpr_count"] - b["vgpr_count"]) <= 8, (nw, a, b)
