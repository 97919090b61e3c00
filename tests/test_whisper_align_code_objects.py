"""Register allocation of the word-alignment kernels, read from the gfx950 code object as tests/test_code_objects.py
reads the towers': no spilled registers and no scratch in any of them."""
import os

import pytest

from test_code_objects import LIB, kernel_notes

KERNELS = ("align_scores_kernel", "align_softmax_kernel", "align_normalize_kernel", "align_median_mean_kernel", "dtw_kernel")


def _short(name):
    """the kernel's name without return type, namespace and argument list"""
    return name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]


def test_alignment_kernels_do_not_spill(tmp_path):
    path = os.path.join(LIB, "whisper_align.o")
    if not os.path.isfile(path):
        pytest.skip("whisper_align.o not built (run __graft_entry__.build())")
    notes = {_short(k): v for k, v in kernel_notes(path, str(tmp_path)).items()}
    assert sorted(notes) == sorted(KERNELS), sorted(notes)
    for k in KERNELS:
        v = notes[k]
        print(k, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
