"""transcribe_many() on scripted decode results (no GPU): the same per-file scripts drive transcribe() through a scripted decode() and
transcribe_many() through a scripted decode_many(); the dicts must be equal, and the recorded rounds say which windows were in flight
together.  Also the ABI of the per-row entry points."""
import os
import re
import types

import pytest
import torch

from hirest_amd import _lib, synth, whisper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("hirest_attention_f32_decode_inplace_rows", "hirest_whisper_step_tail_rows", "hirest_whisper_step_rows_workspace_bytes",
               "hirest_whisper_decode_step_rows")


def test_rows_entries_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hirest_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared <= set(_lib.EXPORTS) | {"hirest_abi_version"}, declared - set(_lib.EXPORTS)
    assert lib.hirest_abi_version() == 4 and "#define HIREST_ABI_VERSION 4" in text
    # the record is 8 words, and the binding lays it out as the header does
    fields = re.search(r"typedef struct hirest_whisper_row_ctl \{(.*?)\} hirest_whisper_row_ctl;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[2\])?;", fields) == ["position", "step", "max_steps", "draw_row", "seed", "temperature", "reserved"]
    ctl = whisper.new_row_ctl([(7, 2, 24, 3, 0xFFFFFFF0, 0.4), (-1, 0, 1, 0, 5, 0.0)], "cpu")
    assert ctl.shape == (2, 8) == (2, _lib.WHISPER_ROW_CTL_WORDS) and ctl.dtype == torch.int32
    assert ctl[0, :4].tolist() == [7, 2, 24, 3] and ctl[0, 4].item() == -16 and ctl[0, 5:6].view(torch.float32).item() == pytest.approx(0.4, abs=1e-7)
    assert ctl[1].tolist() == [-1, 0, 1, 0, 5, 0, 0, 0]
    # argument checks that need no GPU; the rows' positions take room behind the one-position step's workspace
    assert lib.hirest_whisper_step_tail_rows(None, 0, 1, 4, 0, 8, None, None, None, None, None, None, None, None) == -1
    assert lib.hirest_attention_f32_decode_inplace_rows(None, 0, None, None, 0, 0, None, 1, None, None, 0, None, 1, 1, 1.0, 0.0, 0.0, None) == -1
    desc = _lib.WhisperDecoder()
    desc.layers, desc.heads, desc.hidden, desc.inter, desc.vocab_padded, desc.max_pos = 2, 2, 128, 512, 200, 48
    one, rows = lib.hirest_whisper_step_workspace_bytes(desc, 11, 33), lib.hirest_whisper_step_rows_workspace_bytes(desc, 11, 33)
    assert rows == one + 256 and lib.hirest_whisper_step_rows_workspace_bytes(desc, 0, 33) == 0
    assert lib.hirest_whisper_decode_step_rows(desc, 11, None, None, None, None, 48, None, 1, 33, None, None, None, 0, None) == -1


@pytest.fixture(scope="module")
def tok():
    return synth.whisper_tokenizer(50256)


def _stub_model():
    return types.SimpleNamespace(dims={"n_mels": 80, "n_audio_ctx": 1500}, is_multilingual=False, device=torch.device("cpu"), tokenizer=None)


def _res(tok, tokens, temperature=0.0, avg_logprob=-0.2, no_speech_prob=0.01, compression_ratio=1.2):
    return whisper.DecodingResult(tokens=list(tokens), text=tok.decode(tokens), avg_logprob=avg_logprob, no_speech_prob=no_speech_prob,
                                  temperature=temperature, compression_ratio=compression_ratio)


def _mel(file, frames):
    """a zero spectrogram of ``frames`` content frames; row 0 carries the frame number and row 1 the file, so a stub sees which window it got"""
    mel = torch.zeros((80, frames + 3000))
    mel[0] = torch.arange(frames + 3000, dtype=torch.float32)
    mel[1] = float(file)
    return mel


def _scripts(tok):
    tb, a, b = tok.timestamp_begin, tok.encode(" the"), tok.encode(" thing")
    whole = [tb] + a + [tb + 1500]                                     # one segment over the whole window
    pair = [tb] + a + [tb + 100, tb + 100] + b + [tb + 250, tb + 250]  # two closed pairs: seek moves to frame 500
    # file 0: 6000 frames, two plain windows — it ends two rounds before the others
    f0 = (6000, [_res(tok, whole), _res(tok, whole)])
    # file 1: 9000 frames; the first window stays unlikely and silent at both temperatures (skipped), the second is too repetitive and
    # falls back to 0.6 — above 0.5: the third gets no prompt
    f1 = (9000, [_res(tok, whole, 0.0, avg_logprob=-1.2, no_speech_prob=0.9), _res(tok, whole, 0.6, avg_logprob=-1.2, no_speech_prob=0.9),
                 _res(tok, whole, 0.0, compression_ratio=3.0), _res(tok, whole, 0.6), _res(tok, whole)])
    # file 2: 3500 frames: pairs up to frame 500, then the rest
    f2 = (3500, [_res(tok, pair), _res(tok, whole)])
    # file 3: 3000 frames, one window
    f3 = (3000, [_res(tok, whole)])
    return [f0, f1, f2, f3]


def _run_single(monkeypatch, tok, file, frames, script, **kw):
    calls, it = [], iter(script)

    def fake_decode(model, segment, options):
        assert tuple(segment.shape) == (80, 3000)
        calls.append((int(segment[1, 0]), int(segment[0, 0]), options.temperature, list(options.prompt)))
        return next(it)
    monkeypatch.setattr(whisper, "decode", fake_decode)
    out = whisper.transcribe(_stub_model(), _mel(file, frames), tokenizer=tok, **kw)
    assert next(it, None) is None
    return out, calls


def _run_many(monkeypatch, tok, scripts, files_in_flight, **kw):
    rounds, its = [], [iter(s) for _, s in scripts]

    def fake_decode_many(model, segments, options):
        assert len(segments) == len(options) and all(tuple(s.shape) == (80, 3000) for s in segments)
        rounds.append([(int(s[1, 0]), int(s[0, 0]), o.temperature, list(o.prompt)) for s, o in zip(segments, options)])
        return [next(its[int(s[1, 0])]) for s in segments]

    def no_decode(*a, **k):
        raise AssertionError("transcribe_many decodes through decode_many")
    monkeypatch.setattr(whisper, "decode_many", fake_decode_many)
    monkeypatch.setattr(whisper, "decode", no_decode)
    out = whisper.transcribe_many(_stub_model(), [_mel(i, frames) for i, (frames, _) in enumerate(scripts)], files_in_flight=files_in_flight,
                                  tokenizer=tok, **kw)
    assert all(next(it, None) is None for it in its), "transcribe_many made fewer decode calls than scripted"
    return out, rounds


def test_transcribe_many_equals_transcribe_on_scripts(monkeypatch, tok):
    kw = dict(temperature=(0.0, 0.6), best_of=5, no_speech_threshold=0.6, logprob_threshold=-1.0)
    scripts = _scripts(tok)
    want, calls = zip(*[_run_single(monkeypatch, tok, i, frames, script, **kw) for i, (frames, script) in enumerate(scripts)])
    # what the scripts were written to exercise, seen in transcribe()'s own calls
    assert [(c[1], c[2]) for c in calls[1]] == [(0, 0.0), (0, 0.6), (3000, 0.0), (3000, 0.6), (6000, 0.0)]      # fallbacks in file 1 only
    assert [(s["seek"], s["temperature"]) for s in want[1]["segments"]] == [(3000, 0.6), (6000, 0.0)]            # its first window was skipped
    assert calls[1][4][3] == [] and calls[0][1][3] != []              # the prompt is reset after 0.6, and carried over otherwise
    assert [(c[1], c[2]) for c in calls[2]] == [(0, 0.0), (500, 0.0)]
    assert all(c[2] == 0.0 for f in (0, 2, 3) for c in calls[f])
    got, rounds = _run_many(monkeypatch, tok, scripts, 3, **kw)
    assert list(got) == list(want)
    # (file, seek, temperature) in flight together: file 0 ends after round 2 and file 3 takes its slot; a fallback is the file's next request
    assert [[r[:3] for r in rnd] for rnd in rounds] == [
        [(0, 0, 0.0), (1, 0, 0.0), (2, 0, 0.0)],
        [(0, 3000, 0.0), (1, 0, 0.6), (2, 500, 0.0)],
        [(3, 0, 0.0), (1, 3000, 0.0)],
        [(1, 3000, 0.6)],
        [(1, 6000, 0.0)]]
    # every request is the one transcribe() made for that file, in that file's order
    for f in range(4):
        assert [r for rnd in rounds for r in rnd if r[0] == f] == list(calls[f])
    # any number in flight gives the same dicts; one in flight is one window per round, file after file
    for n in (1, 2, 8):
        got_n, rounds_n = _run_many(monkeypatch, tok, scripts, n, **kw)
        assert list(got_n) == list(want) and max(len(r) for r in rounds_n) == min(n, 4)
    assert [r[0][0] for r in _run_many(monkeypatch, tok, scripts, 1, **kw)[1]] == [0, 0, 1, 1, 1, 1, 1, 2, 2, 3]


def test_transcribe_many_edges(monkeypatch, tok):
    assert whisper.transcribe_many(_stub_model(), [], tokenizer=tok) == []
    with pytest.raises(ValueError, match="files_in_flight"):
        whisper.transcribe_many(_stub_model(), [], files_in_flight=0, tokenizer=tok)
    # a file without content is done before its first request and does not hold a slot
    got, rounds = _run_many(monkeypatch, tok, [(0, []), (3000, _scripts(tok)[3][1])], 1, temperature=0.0)
    assert got[0] == {"text": "", "segments": [], "language": "en"} and len(got[1]["segments"]) == 1 and [len(r) for r in rounds] == [1]
    assert whisper.FILES_IN_FLIGHT >= 1
