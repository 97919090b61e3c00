"""The graph-replayed Whisper decoding loop, what of it needs no GPU: how the ``graph`` keyword and HIREST_WHISPER_GRAPH
resolve, that ``graph=True`` has no CPU path either, the counted tail's declaration and argument checks, and the throttle — a pure
function of (chunks issued, pinned stamp) — over every stamp a 3-chunk loop can show."""
import math
import os
import re

import pytest
import torch

from hirest_amd import _lib, build, synth, whisper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_counted_tail_declared_bound_and_checked():
    build.build(verbose=False)
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hirest_hip.h")).read(), flags=re.S)
    name = "hirest_whisper_step_tail_rows_counted"
    assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.EXPORTS
    plain, counted = _lib._SIGNATURES["hirest_whisper_step_tail_rows"][1], _lib._SIGNATURES[name][1]
    assert len(plain) == len(counted) and [i for i, (a, b) in enumerate(zip(plain, counted)) if a is not b] == [4]      # `call` became `count`
    assert lib.hirest_whisper_step_tail_rows_counted(None, 0, 1, 4, None, 8, None, None, None, None, None, None, None, None) == -1
    p = _lib.WhisperTailParams()
    assert lib.hirest_whisper_step_tail_rows_counted(1 << 20, 4, 1, 4, None, 8, p, 1 << 21, 1 << 22, 1 << 23, 1 << 24, None, None, None) == -1


def test_keyword_and_environment(monkeypatch):
    monkeypatch.delenv("HIREST_WHISPER_GRAPH", raising=False)
    assert whisper.resolve_graph(None) is False and whisper.resolve_graph(True) is True and whisper.resolve_graph(False) is False
    for value, want in (("1", True), ("0", False), ("", False), (" 1 ", True)):
        monkeypatch.setenv("HIREST_WHISPER_GRAPH", value)
        assert whisper.resolve_graph(None) is want, value
        assert whisper.resolve_graph(False) is False and whisper.resolve_graph(True) is True           # the keyword wins
    assert whisper.DECODE_GRAPH_CHUNK == 8 and whisper.DECODE_ARENAS >= 2
    # the options and the result carry nothing of it
    assert "graph" not in {f.name for f in whisper.dataclasses.fields(whisper.DecodingOptions)}
    assert "graph" not in {f.name for f in whisper.dataclasses.fields(whisper.DecodingResult)}


def cpu_model():
    cfg, eot, seed, _ = synth.WHISPER_DEC_CASES["p"]
    enc = synth.whisper_encoder_state_dict(cfg, 73)
    sd = {**{"encoder." + k: v for k, v in enc.items()}, **synth.whisper_decoder_state_dict(cfg, seed, eot, synth.WHISPER_DEC_EOT_BIAS["p"])}
    return whisper.Whisper(cfg, sd, synth.whisper_tokenizer(eot)), synth.whisper_audio_states(cfg, 1, seed + 100)


def test_no_cpu_path_with_graph_either(monkeypatch):
    monkeypatch.delenv("HIREST_WHISPER_GRAPH", raising=False)
    m, xa = cpu_model()
    assert m.graph_stats() == {"captures": 0, "replays": 0, "eager_steps": 0}
    with pytest.raises(RuntimeError, match="MI355X only") as e:
        m.decoder(torch.zeros((1, 2), dtype=torch.int64), xa)         # the decoder's own refusal
    want = str(e.value)
    for call in (lambda: whisper.decode(m, xa[0], whisper.DecodingOptions(), graph=True), lambda: m.decode(xa[0], graph=True),
                 lambda: whisper.decode_many(m, xa, whisper.DecodingOptions(), graph=True)):
        with pytest.raises(RuntimeError, match="MI355X only") as e:
            call()
        assert str(e.value) == want
    monkeypatch.setenv("HIREST_WHISPER_GRAPH", "1")                   # and where the environment turns it on
    with pytest.raises(RuntimeError, match="MI355X only"):
        whisper.decode(m, xa[0], whisper.DecodingOptions())
    monkeypatch.delenv("HIREST_WHISPER_GRAPH")
    mel = torch.zeros((m.dims["n_mels"], 3000 + 3000))
    for fn, arg in ((whisper.transcribe, mel), (whisper.transcribe_many, [mel])):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(m, arg, graph=True)
    assert m.graph_stats() == {"captures": 0, "replays": 0, "eager_steps": 0}


def run_throttle(chunk, max_steps, steps):
    """the replaying loop against a device that has landed everything issued to it whenever the host looks (the fastest device), and
    against one that lands one tail per look (the slowest that still moves): -> chunks replayed.  ``steps``: the tail after which no
    row is active."""
    counts = []
    for eager_device in (True, False):
        issued, landed, looks = 0, 1, 0
        while True:
            enqueued = 1 + issued * chunk
            landed = enqueued if eager_device else min(landed + 1, enqueued)
            stamp = (landed << 1) | int(landed >= steps)
            act = whisper.graph_throttle(issued, stamp, chunk, max_steps)
            looks += 1
            assert looks < 10000
            if act == "stop":
                # every tail the loop needs is enqueued: the one that ends the last row, or the last one a row has room for
                assert enqueued >= min(steps, max_steps), (chunk, max_steps, steps, issued)
                break
            if act == "wait":
                assert issued >= 2 and landed < 1 + (issued - 1) * chunk and not eager_device
                continue
            assert act == "issue" and (issued < 2 or landed >= 1 + (issued - 1) * chunk)
            issued += 1
        counts.append(issued)
    return counts


def test_throttle_over_every_stamp_of_a_three_chunk_loop():
    chunk, max_steps = 4, 1 + 3 * 4                                   # iteration 0 and three chunks
    T = whisper.graph_throttle
    for issued in range(0, 4):
        enqueued = 1 + issued * chunk
        for landed in range(0, enqueued + 1):
            for done in (0, 1):
                act = T(issued, (landed << 1) | done, chunk, max_steps)
                if done or issued == 3:                               # no row is active, or every tail of max_steps is enqueued
                    want = "stop"
                elif issued == 2 and landed < 1 + chunk:              # two chunks out and the first has not landed
                    want = "wait"
                else:
                    want = "issue"
                assert act == want, (issued, landed, done, act)
    assert T(0, 0, chunk, 1) == "stop"                                # one step: iteration 0 was all of it
    assert T(5, (max_steps << 1) | 0, chunk, max_steps) == "stop"     # max_steps tails have landed
    for bad in ((-1, 0, 4, 8), (0, -2, 4, 8), (0, 0, 0, 8), (0, 0, 4, 0)):
        with pytest.raises(ValueError):
            T(*bad)
    # whole loops: wasted chunks stay within two, and the loop never stops short of the tail it needs
    for chunk in (1, 2, 4, 8):
        for max_steps in (1, 2, chunk, chunk + 1, chunk + 2, 3 * chunk + 1, 3 * chunk + 2):
            for steps in range(1, max_steps + 1):
                for n in run_throttle(chunk, max_steps, steps):
                    assert n <= math.ceil(steps / chunk) + 2, (chunk, max_steps, steps, n)
