"""Register allocation of the streaming attention kernel, read from the gfx950 code object as tests/test_code_objects.py
reads the towers': attention_long.o holds exactly the kernel named, with no spilled registers and no scratch."""
import os

import pytest

from test_code_objects import LIB, kernel_notes

KERNELS = ("attention_long_kernel",)


def _short(name):
    """the kernel's name without return type, namespace and argument list"""
    return name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]


def test_long_attention_kernel_does_not_spill(tmp_path):
    path = os.path.join(LIB, "attention_long.o")
    if not os.path.isfile(path):
        pytest.skip("attention_long.o not built (run __graft_entry__.build())")
    notes = {_short(k): v for k, v in kernel_notes(path, str(tmp_path)).items()}
    assert sorted(notes) == sorted(KERNELS), sorted(notes)
    for k in KERNELS:
        v = notes[k]
        print(k, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        # four workgroups of four waves per CU: at most 128 registers per lane (vector and accumulation registers are one file on gfx950)
        assert v["vgpr_count"] <= 128, (k, v)
