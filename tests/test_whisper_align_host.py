"""Word-level timestamps, the host side: the numpy restatement itself (dtw against brute force, the median filter's
padding rules), the tokenizer's word split, merge_punctuations, the hand-out of words to segments, and transcribe(word_timestamps=)
on scripted decode results."""
import copy
import re
import os
import types

import numpy as np
import pytest
import torch

import _whisper_align_ref as A
from hirest_amd import _lib, synth, whisper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hirest_whisper_alignment_workspace_bytes", "hirest_whisper_alignment_matrix", "hirest_median_filter_mean_f32",
           "hirest_dtw_workspace_bytes", "hirest_dtw_f32")


def test_entries_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hirest_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hirest_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "whisper_align.hip" in __import__("hirest_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.hirest_whisper_alignment_workspace_bytes(72, 220, 1500) == 72 * 220 * 1500 * 4
    # argument checks that need no GPU: none of these launches
    assert lib.hirest_whisper_alignment_matrix(None, 0, None, 1, 1, 1, None, 1, 1, 1, 1.0, 7, 0, 1, None, None, 0, None) == -1
    assert lib.hirest_median_filter_mean_f32(None, 1, 1, 1, 7, 0, 1, None, None) == -1
    assert lib.hirest_dtw_f32(None, 1, None, 0, None) == -1
    p = (_lib.DtwProblem * 1)()
    p[0].N, p[0].M = 256, 4096
    assert lib.hirest_dtw_workspace_bytes(p, 1) == 256 * 256 * 4 + (256 + 4096) * 8
    for N, M in ((0, 5), (257, 5), (5, 0), (5, 4097)):
        p[0].N, p[0].M = N, M
        assert lib.hirest_dtw_workspace_bytes(p, 1) == 0


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind", ["real", "integer"])
def test_reference_dtw_against_brute_force(kind):
    paths = A.monotone_paths(4, 5)
    assert len(paths) == 129                                          # the Delannoy number D(3, 4)
    for seed in range(12):
        u = synth.uniform_pm1(f"align.dtw.{kind}", 20, seed).reshape(4, 5)
        x = np.round(u * 2.0) if kind == "integer" else u
        ti, tj, cost = A.dtw(x, return_cost=True)
        got = list(zip(ti.tolist(), tj.tolist()))
        costs = [A.path_cost(x, p) for p in paths]
        best = min(costs)
        assert got in paths and abs(cost[-1, -1] - A.path_cost(x, got)) <= 1e-12         # the path is the one the cost was built along
        if kind == "real":                                            # no ties: the rule takes the smallest predecessor, the path is the optimum
            assert abs(A.path_cost(x, got) - best) <= 1e-12 and sum(abs(c - best) <= 1e-12 for c in costs) == 1
        else:                                                         # ties: see test_reference_dtw_tie_rule — never below the optimum
            assert A.path_cost(x, got) >= best


def test_reference_dtw_tie_rule():
    """all costs equal: the diagonal is taken only when strictly smallest, then up only when strictly smallest, else left — so the path
    runs down the first column and then along the last row"""
    ti, tj = A.dtw(np.zeros((2, 2)))
    assert list(zip(ti.tolist(), tj.tolist())) == [(0, 0), (1, 0), (1, 1)]
    ti, tj = A.dtw(np.zeros((3, 3)))
    assert list(zip(ti.tolist(), tj.tolist())) == [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)]
    ti, tj = A.dtw(1.0 - 2.0 * np.eye(3))                                        # a strictly better diagonal is taken
    assert list(zip(ti.tolist(), tj.tolist())) == [(0, 0), (1, 1), (2, 2)]
    # The rule is a definition, not an optimum: where the diagonal and the upper predecessor tie below the left one, neither is
    # "strictly smallest" and the LEFT one is taken.  At cell (1, 1): c0 = 1, c1 = 1 + 0, c2 = 1 + 5 -> 6 + x[1, 1], path through (1, 0).
    ti, tj, cost = A.dtw(np.array([[1.0, 0.0], [5.0, 2.0]]), return_cost=True)
    assert list(zip(ti.tolist(), tj.tolist())) == [(0, 0), (1, 0), (1, 1)] and cost.tolist() == [[1.0, 1.0], [6.0, 8.0]]
    ti, tj = A.dtw(np.zeros((1, 4)), dtype=np.float32)
    assert ti.tolist() == [0] * 4 and tj.tolist() == [0, 1, 2, 3]


def test_reference_median_filter():
    x = np.array([[5.0, 1.0, 4.0, 2.0, 3.0, 9.0]])
    # width 3, reflect: the padded row is 1 | 5 1 4 2 3 9 | 3
    assert A.median_filter(x, 3).tolist() == [[1.0, 4.0, 2.0, 3.0, 3.0, 3.0]]
    # width 5: 4 1 | 5 1 4 2 3 9 | 3 2
    assert A.median_filter(x, 5).tolist() == [[4.0, 2.0, 3.0, 3.0, 3.0, 3.0]]
    assert A.median_filter(x, 1) is x or np.array_equal(A.median_filter(x, 1), x)
    short = np.array([[3.0, 1.0, 2.0]])
    assert A.median_filter(short, 7) is short                         # 3 <= 7 // 2: the early return
    four = np.array([[3.0, 1.0, 2.0, 0.0]])
    assert A.median_filter(four, 7).shape == (1, 4) and A.median_filter(four, 7) is not four


# ---------------------------------------------------------------------------------------------------------------- words
@pytest.fixture(scope="module")
def tok():
    return synth.whisper_tokenizer(100)


def test_split_to_word_tokens(tok):
    text = " the thing, in a -x"
    ids = tok.encode(text)
    words, word_tokens = tok.split_to_word_tokens(ids + [tok.eot])
    assert words == [" the", " thing", ",", " in", " a", " -x", "<|endoftext|>"]
    assert [t for w in word_tokens for t in w] == ids + [tok.eot] and word_tokens[-1] == [tok.eot]
    assert [tok.decode(w) for w in word_tokens] == words
    # the first piece opens a word whatever it is; a piece without a space continues the word
    words, word_tokens = tok.split_to_word_tokens(tok.encode("ab c"))
    assert words == ["ab", " c"] and [len(w) for w in word_tokens] == [2, 2]
    # on unicode boundaries (languages written without spaces): every complete character run of a token is a word
    zh = tok.with_language("zh", None)
    words, word_tokens = zh.split_to_word_tokens(tok.encode("ab c"))
    assert words == ["a", "b", " ", "c"] and all(len(w) == 1 for w in word_tokens)
    big = synth.whisper_tokenizer(50256)                              # bytes of one character in separate tokens stay together
    ids = big.encode(" é♪")
    assert len(ids) > 2
    words, word_tokens = big.split_tokens_on_unicode(ids)
    assert "".join(words) == " é♪" and "�" not in "".join(words) and [t for w in word_tokens for t in w] == ids


def test_merge_punctuations():
    W = whisper.WordTiming
    a = [W(" (", [1], 0.0, 0.1, 0.5), W(" the", [2], 0.1, 0.4, 0.6), W(",", [3], 0.4, 0.5, 0.7), W(" thing", [4, 5], 0.5, 0.9, 0.8),
         W(".", [6], 0.9, 1.0, 0.9), W(")", [7], 1.0, 1.1, 0.9)]
    whisper.merge_punctuations(a)
    assert [w.word for w in a] == ["", " ( the,", "", " thing.)", "", ""]
    assert [w.tokens for w in a] == [[], [1, 2, 3], [], [4, 5, 6, 7], [], []]
    assert (a[1].start, a[1].end, a[3].start, a[3].end) == (0.1, 0.4, 0.5, 0.9)       # the joined word keeps its own times
    b = [W(" a", [1], 0.0, 0.1, 0.5), W(" -", [2], 0.1, 0.2, 0.5), W(" b", [3], 0.2, 0.3, 0.5)]
    whisper.timing.merge_punctuations(b, "-", "")
    assert [w.word for w in b] == [" a", "", " - b"]
    c = [W(" a ", [1], 0.0, 0.1, 0.5), W(".", [2], 0.1, 0.2, 0.5)]      # a word that ends with a space takes nothing
    whisper.merge_punctuations(c)
    assert [w.word for w in c] == [" a ", "."]


def _stub_model():
    return types.SimpleNamespace(dims={"n_mels": 80, "n_audio_ctx": 1500}, is_multilingual=False, device=torch.device("cpu"), tokenizer=None)


def test_words_go_to_segments_by_token_count(monkeypatch, tok):
    tb = tok.timestamp_begin
    first, second = tok.encode(" the thing,"), tok.encode("in a")      # the second segment starts without a space
    segments = [{"seek": 500, "start": 5.0, "end": 6.0, "tokens": [tb] + first + [tb + 50], "text": " the thing,"},
                {"seek": 500, "start": 6.0, "end": 7.5, "tokens": [tb + 50] + second + [tb + 125], "text": "in a"}]
    seen = {}

    def fake(model, tokenizer, text_tokens, mel, num_frames, **kw):
        seen.update(text_tokens=list(text_tokens), num_frames=num_frames, kw=kw)
        words, word_tokens = whisper._split_words(tokenizer, text_tokens, kw.get("segment_lengths"))
        n = len(words) - 1
        return [whisper.WordTiming(w, list(t), 0.5 * i - 0.25, 0.5 * i + 0.25, 0.5) for i, (w, t) in enumerate(zip(words[:n], word_tokens[:n]))]
    monkeypatch.setattr(whisper, "find_alignment", fake)
    whisper.add_word_timestamps(segments, _stub_model(), tok, torch.zeros((80, 3000)), 2400)
    assert seen["text_tokens"] == first + second and seen["num_frames"] == 2400 and seen["kw"]["segment_lengths"] == [len(first), len(second)]
    # words: " the" [-0.25, 0.25], " thing" [0.25, 0.75] with "," [0.75, 1.25] merged into it | "in" [1.25, 1.75], " a" [1.75, 2.25]
    w0, w1 = segments[0]["words"], segments[1]["words"]
    assert [w["word"] for w in w0] == [" the", " thing,"] and [w["word"] for w in w1] == ["in", " a"]
    assert "".join(w["word"] for w in w0) == segments[0]["text"] and "".join(w["word"] for w in w1) == segments[1]["text"]
    # offset 5 s, the first word's start clipped to the segment's start, the last word's end to the segment's end
    assert [(w["start"], w["end"]) for w in w0] == [(5.0, 5.25), (5.25, 5.75)]
    assert [(w["start"], w["end"]) for w in w1] == [(6.25, 6.75), (6.75, 7.25)]
    assert all(set(w) == {"word", "start", "end", "probability"} for w in w0 + w1)
    segments[1]["end"] = 7.0
    whisper.add_word_timestamps(segments, _stub_model(), tok, torch.zeros((80, 3000)), 2400)
    assert segments[1]["words"][-1]["end"] == 7.0


def test_find_alignment_of_nothing_is_empty(tok):
    assert whisper.find_alignment(_stub_model(), tok, [], torch.zeros((80, 3000)), 3000) == []


# ---------------------------------------------------------------------------------------------------------------- transcribe
def _res(tok, tokens, avg_logprob=-0.2, no_speech_prob=0.01):
    return whisper.DecodingResult(tokens=list(tokens), text=tok.decode(tokens), avg_logprob=avg_logprob, no_speech_prob=no_speech_prob,
                                  temperature=0.0, compression_ratio=1.2)


def _run(monkeypatch, tok, script, frames, **kw):
    it, aligned = iter(script), []

    def fake_decode(model, segment, options):
        return next(it)

    def fake_find_alignment(model, tokenizer, text_tokens, mel, num_frames, **kw_):
        aligned.append((list(text_tokens), tuple(mel.shape), float(mel[0, 0]), num_frames))
        words, word_tokens = whisper._split_words(tokenizer, text_tokens, kw_.get("segment_lengths"))
        return [whisper.WordTiming(w, list(t), 0.1 * i, 0.1 * i + 0.1, 0.9) for i, (w, t) in enumerate(zip(words[:-1], word_tokens[:-1]))]
    monkeypatch.setattr(whisper, "decode", fake_decode)
    monkeypatch.setattr(whisper, "find_alignment", fake_find_alignment)
    mel = torch.zeros((80, frames + 3000))
    mel[0] = torch.arange(frames + 3000, dtype=torch.float32)
    out = whisper.transcribe(_stub_model(), mel, tokenizer=tok, temperature=0.0, **kw)
    assert next(it, None) is None
    return out, aligned


def test_transcribe_word_timestamps(monkeypatch, tok):
    tb, a, b, c = tok.timestamp_begin, tok.encode(" the"), tok.encode(" thing."), tok.encode(" in")
    first = [tb] + a + [tb + 100, tb + 100] + b + [tb + 250, tb + 250]             # two closed pairs: two segments, seek to frame 500
    silent = _res(tok, [tb] + a + [tb + 10], avg_logprob=-1.2, no_speech_prob=0.9)  # skipped as no-speech
    third = [tb] + c + [tb + 40]
    script = lambda: [_res(tok, first), silent, _res(tok, third)]
    off, aligned = _run(monkeypatch, tok, script(), frames=5000, logprob_threshold=None)
    assert aligned == [] and all("words" not in s for s in off["segments"])
    on, aligned = _run(monkeypatch, tok, script(), frames=5000, logprob_threshold=None, word_timestamps=True)
    # once per settled window that has segments, on that window's frames; not for the window skipped as no-speech
    assert aligned == [(a + b, (80, 3000), 0.0, 3000), (c, (80, 3000), 3500.0, 1500)]
    assert len(on["segments"]) == len(off["segments"]) == 3
    stripped = copy.deepcopy(on["segments"])
    for s in stripped:
        del s["words"]
    assert stripped == off["segments"] and on["text"] == off["text"]
    assert [[w["word"] for w in s["words"]] for s in on["segments"]] == [[" the"], [" thing."], [" in"]]
    assert on["segments"][2]["words"][0]["start"] == 35.0             # the window's offset is added
    assert on["segments"][1]["words"][0]["start"] == 2.0              # 0.1 s, clipped to the segment's start


def test_transcribe_word_timestamps_of_a_last_sliver(monkeypatch, tok):
    """a last window of one frame has no num_frames // 2 keys: it is aligned over one key"""
    tb, a = tok.timestamp_begin, tok.encode(" the")
    res = lambda: _res(tok, [tb] + a + [tb + 1500])
    out, aligned = _run(monkeypatch, tok, [res(), res()], frames=3001, word_timestamps=True)
    assert [x[2:] for x in aligned] == [(0.0, 3000), (3000.0, 2)] and len(out["segments"]) == 2


def test_transcribe_word_timestamps_punctuation_sets(monkeypatch, tok):
    tb, b = tok.timestamp_begin, tok.encode(" thing.")
    out, _ = _run(monkeypatch, tok, [_res(tok, [tb] + b + [tb + 1500])], frames=3000, word_timestamps=True, append_punctuations="")
    assert [w["word"] for w in out["segments"][0]["words"]] == [" thing", "."]
