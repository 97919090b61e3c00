"""BERTScore (evaluate.py:294-297) on the host: the byte-level BPE tokenizer against the installed ``tokenizers`` pipeline's recorded
ids (tests/golden/bytebpe.json), the fp64 restatement of the matching (tests/_bertscore_ref.py) against the fixture's triples, the
hirest_bertscore_greedy entry point's declaration and argument checks, evaluate_bert_score's host plan and the loading surface.
No device needed."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bertscore_ref as ref  # noqa: E402
from hirest_amd import bert_score, evaluation, synth  # noqa: E402
from hirest_amd.bytebpe import ByteBPETokenizer, bytes_to_unicode  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def bpe():
    with open(os.path.join(GOLDEN, "bytebpe.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tok(bpe):
    return ByteBPETokenizer(bpe["vocab"], bpe["merges"])


# ------------------------------------------------------------------------------------------------------------ tokenizer

def test_bytes_to_unicode_is_a_printable_bijection():
    t = bytes_to_unicode()
    assert sorted(t) == list(range(256)) and len(set(t.values())) == 256
    assert t[ord("a")] == "a" and t[ord(" ")] == "Ġ" and t[ord("\n")] == "Ċ"


def test_ids_equal_the_tokenizers_pipeline(bpe, tok):
    assert len(bpe["vocab"]) <= 600
    for text, ids, short in zip(bpe["texts"], bpe["ids"], bpe["ids_max8"]):
        assert tok.encode(text, 512) == ids, text
        assert tok.encode(text, 8) == short, text
        assert len(short) <= 8
    assert any(len(i) > 8 for i in bpe["ids"])                  # the truncated column differs from the full one somewhere


def test_empty_string_is_the_two_specials(bpe, tok):
    assert (tok.bos_id, tok.pad_id, tok.eos_id) == (bpe["vocab"]["<s>"], bpe["vocab"]["<pad>"], bpe["vocab"]["</s>"]) == (0, 1, 2)
    assert tok.encode("") == [0, 2]
    assert tok.encode("anything at all", 2) == [0, 2]


def test_merges_file_header_and_pairs_are_accepted(bpe):
    a = ByteBPETokenizer(bpe["vocab"], ["#version: 0.2"] + bpe["merges"] + [""])
    b = ByteBPETokenizer(bpe["vocab"], [tuple(m.split(" ")) for m in bpe["merges"]])
    for text, ids in zip(bpe["texts"], bpe["ids"]):
        assert a.encode(text) == ids and b.encode(text) == ids
    with pytest.raises(ValueError):
        ByteBPETokenizer({"a": 0}, [])                          # no <s> / </s> / <pad>


# ------------------------------------------------------------------------------------------------------------ fp64 restatement

def test_restatement_reproduces_the_fixture_from_its_states():
    g = np.load(os.path.join(GOLDEN, "bertscore_tiny.npz"))
    off = np.zeros(len(g["lens"]) + 1, np.int64)
    off[1:] = np.cumsum(g["lens"])
    assert g["states"].dtype == np.float32 and g["states"].shape == (off[-1], synth.ROBERTA_TINY["hidden_size"])
    got = ref.greedy(g["states"], off, ref.special_weights(off), g["cand"], g["ref"])
    # the stored states are the fp64 model's, rounded to fp32: 6e-8 relative per element
    assert np.abs(got - g["triples"]).max() <= 1e-6
    # the zero rules: an empty candidate has P = F = 0 and its R is still computed; an empty reference likewise
    lens = g["lens"] - 2
    for p, (a, b) in enumerate(zip(g["cand"], g["ref"])):
        P, R, F = got[p]
        if lens[a] == 0:
            assert P == 0.0 and F == 0.0 and R > 0
        if lens[b] == 0:
            assert R == 0.0 and F == 0.0 and P > 0
        if a == b:
            assert abs(P - 1) < 1e-12 and abs(R - 1) < 1e-12 and abs(F - 1) < 1e-12
    assert lens[g["cand"][0]] == 0 and lens[g["ref"][0]] == 4 and 0 < got[0, 1] < 1     # R against the two specials alone
    assert np.isnan(ref.greedy(g["states"], off, ref.special_weights(off), [0, len(lens)], [-1, 0])).all()


def test_fixture_sentences_tokenize_to_the_fixture_ids(tok):
    g = np.load(os.path.join(GOLDEN, "bertscore_tiny.npz"))
    maxlen = synth.ROBERTA_TINY["max_position_embeddings"] - synth.ROBERTA_TINY["pad_token_id"] - 1
    rows = np.split(g["ids"], np.cumsum(g["lens"])[:-1])
    assert max(g["lens"]) == maxlen == 66
    for text, row in zip(g["texts"], rows):
        assert tok.encode(str(text).strip(), maxlen) == row.tolist()


# ------------------------------------------------------------------------------------------------------------ C entry point

@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_declared_and_exported(lib):
    from hirest_amd import _lib
    hdr = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    assert "int hirest_bertscore_greedy(const float* states, int64_t ld, int32_t D, const int32_t* seq_off, int32_t n_seq," in hdr
    assert "hirest_bertscore_greedy" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["hirest_bertscore_greedy"][1]) == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hirest_bertscore_greedy")
    assert "bertscore.hip" in __import__("hirest_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.hirest_abi_version() == 4


def test_argument_errors_without_gpu(lib):
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is rejected before anything is enqueued
    ok = dict(states=p, ld=64, D=64, seq_off=p, n_seq=3, w=p, cand=p, ref=p, n_pairs=2, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.hirest_bertscore_greedy(a["states"], a["ld"], a["D"], a["seq_off"], a["n_seq"], a["w"], a["cand"], a["ref"],
                                           a["n_pairs"], a["out"], None)
    for bad in (dict(states=None), dict(seq_off=None), dict(w=None), dict(cand=None), dict(ref=None), dict(out=None),
                dict(D=0, ld=0), dict(D=2, ld=4), dict(D=-4), dict(D=6, ld=8), dict(D=66, ld=68), dict(ld=60), dict(ld=66),
                dict(n_seq=0), dict(n_seq=-1), dict(n_pairs=-1)):
        assert call(**bad) == -1, bad
    assert call(n_pairs=0) == 0           # nothing to score: success, nothing launched


# ------------------------------------------------------------------------------------------------------------ host plan

GT = {"v1.mp4": {"captions": [{"sentence": "Crack The Eggs", "start": 0, "end": 3}, {"sentence": "Whisk", "start": 3, "end": 5}]},
      "v2.mp4": {"captions": [{"sentence": "WHISK", "start": 0, "end": 2}]},
      "v3.mp4": {"captions": []},
      "v4.mp4": {"captions": [{"sentence": "Paint the wall", "start": 1, "end": 2}]}}
PRED = {"v1.mp4": {"captions": [{"sentence": "crack the EGGS"}, {"sentence": "Stir"}]},
        "v2.mp4": {"captions": [{"sentence": "Stir"}]},
        "v3.mp4": {"captions": []},
        "v4.mp4": {"captions": [{"sentence": "paint the wall"}]}}
CATS = {"v1.mp4": "Food", "v2.mp4": "Food", "v3.mp4": "Pets", "v4.mp4": "Home"}


class StubScorer:
    """F of a pair = a number that names the pair: makes the per-category means checkable by hand"""
    def __init__(self):
        self.calls = []

    def to(self, device):
        raise AssertionError("no device was asked for")

    def score_device(self, cands, refs, stats=None):
        self.calls.append((list(cands), list(refs)))
        f = torch.tensor([0.25 * (i + 1) for i in range(len(cands))], dtype=torch.float32)
        return torch.stack([f * 0, f * 0, f], 1)


def test_evaluate_bert_score_host_plan():
    s = StubScorer()
    res = evaluation.evaluate_bert_score(GT, PRED, CATS, s, per_category=True)
    # one call for every pair of every category; both sides lower-cased; candidates are the predictions
    assert s.calls == [(["crack the eggs", "stir", "stir", "paint the wall"], ["crack the eggs", "whisk", "whisk", "paint the wall"])]
    # categories sorted + "all"; "Pets" has a video but no caption and is left out; Total counts videos
    assert list(res) == ["Food", "Home", "all"]
    assert res["Food"] == {"BERTScore_F1": pytest.approx((0.25 + 0.5 + 0.75) / 3), "Total": 2}
    assert res["Home"] == {"BERTScore_F1": 1.0, "Total": 1}
    assert res["all"] == {"BERTScore_F1": pytest.approx(0.625), "Total": 4}
    assert res["Food"]["BERTScore_F1"] == torch.tensor([0.25, 0.5, 0.75]).mean().item()        # the fp32 mean, as f.mean().item()
    assert evaluation.evaluate_bert_score(GT, PRED, CATS, StubScorer(), per_category=False).keys() == {"all"}
    # the same category rules as CLIPScore's plan: one shared walk
    plan = evaluation.clip_score_plan(GT, PRED, None, CATS, per_category=True)
    assert {c: m["Total"] for c, m in plan.categories.items()} == {c: r["Total"] for c, r in res.items()}
    with pytest.raises(KeyError):
        evaluation.evaluate_bert_score(GT, PRED, {k: v for k, v in CATS.items() if k != "v3.mp4"}, StubScorer())
    assert evaluation.evaluate_bert_score({}, {}, {}, StubScorer()) == {}


def test_unique_sentences_are_encoded_once(bpe):
    cfg = synth.ROBERTA_TINY
    scorer = bert_score.BERTScorer(config=cfg, state_dict=synth.roberta_state_dict(cfg, 61, 3), num_layers=3, vocab=bpe["vocab"],
                                   merges=bpe["merges"], device="cpu")
    rows, index = scorer._rows(["stir", "crack the eggs", "stir ", "", "  ", [0, 7, 2], (0, 7, 2)])
    assert index == [0, 1, 0, 2, 2, 3, 3] and len(rows) == 4 and rows[2] == (0, 2)
    with pytest.raises(NotImplementedError, match="several references"):
        scorer._rows([["two", "references"]])


# ------------------------------------------------------------------------------------------------------------ loading surface

def test_hub_name_raises_file_not_found():
    with pytest.raises(FileNotFoundError, match="roberta-large"):
        bert_score.score(["a"], ["b"], lang="en", verbose=True, device="cuda:0")
    with pytest.raises(FileNotFoundError, match="is not a local model directory"):
        bert_score.BERTScorer(model_type="microsoft/deberta-xlarge-mnli")
    with pytest.raises(ValueError):
        bert_score.score(["a"], ["b"])


def test_out_of_scope_options_name_themselves():
    cfg = synth.ROBERTA_TINY
    for kw in ("idf", "all_layers", "rescale_with_baseline"):
        with pytest.raises(NotImplementedError, match=kw):
            bert_score.BERTScorer(config=cfg, state_dict={}, **{kw: True})
        with pytest.raises(NotImplementedError, match=kw):
            bert_score.score(["a"], ["b"], lang="en", **{kw: True})


def test_default_layers():
    assert bert_score.DEFAULT_LAYERS == {("roberta", 24): 17, ("roberta", 12): 10, ("roberta", 6): 5, ("bert", 12): 9, ("bert", 24): 18}
    cfg = synth.ROBERTA_TINY                                     # 4 layers: no default
    with pytest.raises(ValueError, match="num_layers"):
        bert_score.BERTScorer(config=cfg, state_dict=synth.roberta_state_dict(cfg, 1))
    six = dict(cfg, num_hidden_layers=6)
    s = bert_score.BERTScorer(config=six, state_dict=synth.roberta_state_dict(six, 1), device="cpu")
    assert s.num_layers == 5 and s.encoder.layers == 5
    # the layers after the cut are not kept
    assert not any(n.startswith("encoder.layer.5.") for n in s.encoder._names)
    assert any(n.startswith("encoder.layer.4.") for n in s.encoder._names)


def test_model_directory(tmp_path, bpe):
    from safetensors.torch import save_file
    cfg = dict(synth.ROBERTA_TINY, num_hidden_layers=6)
    d = tmp_path / "roberta-six"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    save_file(synth.roberta_state_dict(cfg, 3), str(d / "model.safetensors"))
    (d / "vocab.json").write_text(json.dumps(bpe["vocab"]), encoding="utf-8")
    (d / "merges.txt").write_text("#version: 0.2\n" + "\n".join(bpe["merges"]) + "\n", encoding="utf-8")
    s = bert_score.BERTScorer(model_type=str(d), device="cpu")
    assert s.arch == "roberta" and s.num_layers == 5 and s.max_length == 66
    assert s.encoder.eps == 1e-5 and s.encoder.pos_offset == 2
    assert isinstance(s.tokenizer, ByteBPETokenizer)
    assert s.tokenize("  " + bpe["texts"][2] + " ") == bpe["ids"][2]          # stripped, then <s> ... </s>
    assert s.tokenize("") == [0, 2]
    # no CPU path
    with pytest.raises(RuntimeError, match="MI355X only"):
        s.score(["crack the eggs"], ["whisk"])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            bert_score.score(["crack the eggs"], ["whisk"], model_type=str(d), device="cpu")
    with pytest.raises(ValueError):
        s.score(["a", "b"], ["c"])


def test_bert_directory_uses_wordpiece(tmp_path):
    from safetensors.torch import save_file
    from hirest_amd.wordpiece import WordPieceTokenizer
    cfg = dict(synth.MINILM_TINY, model_type="bert", num_hidden_layers=12)
    d = tmp_path / "bert-twelve"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    save_file({"bert." + k: v for k, v in synth.bert_state_dict(cfg, 3).items()}, str(d / "model.safetensors"))
    with open(os.path.join(GOLDEN, "wordpiece.json"), encoding="utf-8") as f:
        wp = json.load(f)
    (d / "vocab.txt").write_text("\n".join(wp["vocab"]) + "\n", encoding="utf-8")
    s = bert_score.BERTScorer(model_type=str(d), device="cpu")
    assert s.arch == "bert" and s.num_layers == 9 and s.max_length == 64 and s.encoder.pos_offset == 0
    assert isinstance(s.tokenizer, WordPieceTokenizer)
    assert s.tokenize(wp["texts"][2]) == wp["ids"][2]
