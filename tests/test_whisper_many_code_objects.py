"""Register allocation of the per-row decode kernels, read from the gfx950 code objects as tests/test_code_objects.py
reads the towers': no spilled registers, no scratch, and the per-row forms cost what the forms they share their bodies with cost."""
import os

import pytest

from test_code_objects import LIB, kernel_notes


def _short(name):
    """the kernel's name without return type, namespace and argument list (a plain function demangles without "void")"""
    return name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]


def _notes(obj, tmp_path):
    path = os.path.join(LIB, obj)
    if not os.path.isfile(path):
        pytest.skip(f"{obj} not built (run __graft_entry__.build())")
    return {_short(k): v for k, v in kernel_notes(path, str(tmp_path)).items()}


def test_per_row_kernels_do_not_spill(tmp_path):
    joint, dec = _notes("joint.o", tmp_path), _notes("whisper_dec.o", tmp_path)
    pairs = [(joint, "attention_f32_decode_kernel<true, true>", "attention_f32_decode_kernel<true, false>", 4),
             (dec, "whisper_tail_rows_kernel", "whisper_tail_kernel", 8)]
    for notes, rows, base, slack in pairs:
        assert rows in notes and base in notes, sorted(notes)
        for k in (rows, base):
            v = notes[k]
            print(k, v)
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        # (the attention keeps a tile's 32 probabilities wave-uniform: scalar registers that overflow into VGPR lanes, never into memory)
        assert notes[rows]["vgpr_count"] <= notes[base]["vgpr_count"] + slack, (notes[rows], notes[base])
        assert notes[rows]["sgpr_spill_count"] <= notes[base]["sgpr_spill_count"] + 2 * slack, (notes[rows], notes[base])
    for k in ("embed_rows_kernel", "whisper_stamp_rows_kernel"):
        assert dec[k]["vgpr_spill_count"] == 0 and dec[k]["private_segment_fixed_size"] == 0, (k, dec[k])
