"""Host side of the towers (hirest_amd/eva_clip.py, clip.py), no GPU: the parameter tables against the ctypes structs they fill, the
scoped precision switch of both model classes, and what empties the cache of prepared weights."""
import ctypes as C

import pytest
import torch

from hirest_amd import clip, eva_clip, synth


@pytest.fixture(scope="module")
def eva():
    return eva_clip.EVA_CLIP(**synth.EVA_CLIP_TINY)


@pytest.fixture(scope="module")
def openai():
    return clip.CLIP(**synth.OPENAI_VIT_TINY)


def _towers(eva, openai):
    return {"eva.visual": eva.visual, "eva.text": eva.text, "openai.visual": openai.visual, "openai.text": openai._text}


def test_tables_name_every_struct_field_once(eva, openai):
    kinds = {"eva.visual": {"bf16", "fp32", "x3"}, "eva.text": {"bf16", "fp32"}, "openai.visual": {"bf16", "fp32"},
             "openai.text": {"bf16", "fp32"}}
    for name, tower in _towers(eva, openai).items():
        assert set(tower._TABLES) == kinds[name]
        for kind, (desc_cls, rows, block_cls, block_rows) in tower._TABLES.items():
            for struct, table in ((desc_cls, rows), (block_cls, block_rows)):
                pointers = sorted(n for n, t in struct._fields_ if t is C.c_void_p)
                assert sorted(r[0] for r in table) == pointers, (name, kind, struct.__name__)   # each once, none missing, no other
            # what the table does not fill is `blocks` and the scalars (the 'x3' descriptor: a pointer to the fp32 one)
            rest = {"blocks"} | (set(tower._scalars()) if kind != "x3" else {"base"})
            assert rest == {n for n, t in desc_cls._fields_ if t is not C.c_void_p}, (name, kind)
            # a weight matrix is cast, everything else stays fp32: the bf16 and the fp32 descriptor are one walk
            assert all(form in (None, "f32", "w", "wT", "patch", "qkv_bias", "const", "split", "fold0", "fold1", "fold2")
                       for _, form, _ in tuple(rows) + tuple(block_rows))


def test_table_sources_exist(eva, openai):
    from operator import attrgetter
    for name, tower in _towers(eva, openai).items():
        for kind, (_, rows, _, block_rows) in tower._TABLES.items():
            for owner, table in ((tower, rows), (tower._blocks()[0], block_rows)):
                for field, form, src in table:
                    if form == "const":
                        assert len(getattr(tower, src)) == 3
                    elif form is not None:
                        for path in ((src[0], src[2]) if form.startswith("fold") else (src,)):
                            attrgetter(path)(owner)
    assert len(eva.visual._blocks()) == eva.visual.layers and len(openai.visual._blocks()) == openai.visual.layers


def test_struct_by_keyword_rejects_missing_and_unknown_fields():
    from hirest_amd import _lib
    names = [n for n, _ in _lib.BlockWeightsX3._fields_]
    s = eva_clip._struct(_lib.BlockWeightsX3, **{n: i + 1 for i, n in enumerate(names)})
    assert [getattr(s, n) for n in names] == [1, 2, 3, 4]
    with pytest.raises(TypeError):
        eva_clip._struct(_lib.BlockWeightsX3, **{n: 1 for n in names[:-1]})
    with pytest.raises(TypeError):
        eva_clip._struct(_lib.BlockWeightsX3, **{n: 1 for n in names}, qkv_w=1)


@pytest.mark.parametrize("B,limit,near_equal,want", [
    (130, 70, True, [65, 65]), (130, 48, True, [44, 44, 42]), (70, 40, True, [35, 35]), (1030, 1024, True, [515, 515]),
    (5, 2, False, [2, 2, 1]), (1030, 1024, False, [1024, 6]), (3, 1024, False, [3]), (3, 1024, True, [3]), (3, 0, False, [1, 1, 1]),
    (0, 8, True, []), (0, 8, False, [])])
def test_call_sizes(eva, B, limit, near_equal, want):
    tower, got = eva.visual, []
    tower._workspace = None
    spans = tower._run_calls(B, limit, near_equal, lambda n: 16 * n, lambda s, n, ws: got.append((s, n, ws.numel())), torch.device("cpu"))
    assert [n for _, n in spans] == want and [s for s, _ in spans] == [sum(want[:i]) for i in range(len(want))]
    assert got == [(s, n, 16 * max(want)) for s, n in spans]            # one workspace, sized for the largest call
    tower._workspace = None


def test_precision_scope_eva(eva):
    eva.set_precision("bf16")
    with eva.precision_scope(visual="bf16x3"):
        assert (eva.visual.precision, eva.text.precision) == ("bf16x3", "bf16")
        with eva.precision_scope(text="bf16x3"):                         # as set_precision: the text tower has no bf16x3 kernels
            assert (eva.visual.precision, eva.text.precision) == ("bf16x3", "fp32")
        assert (eva.visual.precision, eva.text.precision) == ("bf16x3", "bf16")
    assert (eva.visual.precision, eva.text.precision) == ("bf16", "bf16")
    with pytest.raises(KeyError):
        with eva.precision_scope(visual="fp32", text="fp32"):
            assert (eva.visual.precision, eva.text.precision) == ("fp32", "fp32")
            raise KeyError("inside")
    assert (eva.visual.precision, eva.text.precision) == ("bf16", "bf16")
    for bad in ({"visual": "fp16"}, {"text": "amp"}, {"visual": "bf16", "text": ""}):
        with pytest.raises(ValueError):
            eva.precision_scope(**bad)
    assert (eva.visual.precision, eva.text.precision) == ("bf16", "bf16")


def test_precision_scope_openai(openai):
    openai.set_precision("bf16")
    assert not hasattr(openai, "text")
    with openai.precision_scope(visual="bf16x3", text="fp32"):
        assert (openai.visual.precision, openai._text.precision) == ("fp32", "fp32")
    assert (openai.visual.precision, openai._text.precision) == ("bf16", "bf16")
    openai.set_precision("fp32")
    with pytest.raises(KeyError):
        with openai.precision_scope(text="bf16"):
            assert (openai.visual.precision, openai._text.precision) == ("fp32", "bf16")
            raise KeyError("inside")
    assert (openai.visual.precision, openai._text.precision) == ("fp32", "fp32")
    with pytest.raises(ValueError):
        openai.precision_scope(text="fp16")
    openai.set_precision("bf16")


def test_what_empties_the_cache(eva, openai):
    sentinel = {"bf16": {"device": torch.device("cpu")}}
    for name, tower in _towers(eva, openai).items():
        model = openai if name.startswith("openai") else eva
        resets = {"invalidate": tower.invalidate, "to": lambda: model.to("cpu"), "float": model.float,
                  "load_state_dict": lambda: model.load_state_dict(model.state_dict()), "outside": lambda: setattr(tower, "_prepared", None)}
        for how, reset in resets.items():
            tower._prepared = dict(sentinel)
            reset()
            assert tower._prepared is None, (name, how)
    # a preparation for another device is not served: asking on the CPU finds the cache unusable and refuses to build one
    eva.visual._prepared = {"bf16": {"device": torch.device("cuda:0")}}
    with pytest.raises(RuntimeError, match="MI355X only"):
        eva.visual._prepared_for("bf16", torch.device("cpu"))
    assert eva.visual._prepared == {}
    eva.visual._prepared = None
