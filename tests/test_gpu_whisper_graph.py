"""The capturable decode step and the graph-replayed decoding loop: hirest_whisper_step_tail_rows_counted against
hirest_whisper_step_tail_rows, and decode / decode_many / transcribe with ``graph=True`` against the eager loop of the same process.
Every comparison is ``torch.equal`` or list equality: the replayed loop makes the eager loop's launches on other addresses, and the eager
loop is what tests/test_gpu_whisper_many.py and tests/test_gpu_whisper_dec.py pin to the lock-step loop and to fp64."""
import ctypes as C
import dataclasses
import inspect
import math

import numpy as np
import pytest
import torch

import test_gpu_whisper_dec as S
from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

CANARY = S.CANARY
O = whisper.DecodingOptions


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- the counted tail
def tail_buffers(R, V, eot, dev):
    """rows that start a window (the state's initial value), at positions, budgets, temperatures and seeds of their own: some leave the
    loop at their first, second or third pick, and every fourth is inactive from the start"""
    params, mask = whisper.tail_params(synth.whisper_tokenizer(eot), O(), V, V, 70, 0, dev)
    rows = [(-1 if r % 4 == 3 else 3 + r, 0, 1 + r % 5, r % 5, 11 + r, (0.0, 0.4, 0.9)[r % 3]) for r in range(R)]
    logits = S.seeded("graph.tail", (R, V), V + R, 3.0).to(dev)
    return params, mask, logits, whisper.new_row_ctl(rows, dev), whisper.new_row_state(R, dev)


@pytest.mark.parametrize("V, eot", [(200, 100), (8200, 8000)])
@pytest.mark.parametrize("R", [1, 5, 40])
def test_counted_tail_equals_the_tail_with_its_call_number(R, V, eot, dev):
    lib = _lib.load()
    params, mask, logits, ctl0, state0 = tail_buffers(R, V, eot, dev)
    ld = 8
    new = lambda: dict(ctl=ctl0.clone(), state=state0.clone(), ids=torch.full((R,), -7, dtype=torch.int32, device=dev),
                       tokens=torch.full((R, ld), -7, dtype=torch.int32, device=dev),
                       logprobs=torch.full((R, V), CANARY, dtype=torch.float32, device=dev), stamp=torch.zeros(1, dtype=torch.int32).pin_memory())
    a, b = new(), new()
    count = torch.zeros(3, dtype=torch.int32, device=dev)             # the counter between two guard words
    count[0], count[2] = -5, -6
    stamps = []
    for call in range(3):
        _lib.check(lib.hirest_whisper_step_tail_rows(logits.data_ptr(), V, R, V, call, ld, C.byref(params), a["ctl"].data_ptr(), a["state"].data_ptr(),
                                                     a["ids"].data_ptr(), a["tokens"].data_ptr(), a["logprobs"].data_ptr(), a["stamp"].data_ptr(),
                                                     ops.stream_ptr()), "hirest_whisper_step_tail_rows")
        _lib.check(lib.hirest_whisper_step_tail_rows_counted(logits.data_ptr(), V, R, V, count[1:].data_ptr(), ld, C.byref(params), b["ctl"].data_ptr(),
                                                             b["state"].data_ptr(), b["ids"].data_ptr(), b["tokens"].data_ptr(),
                                                             b["logprobs"].data_ptr(), b["stamp"].data_ptr(), ops.stream_ptr()),
                   "hirest_whisper_step_tail_rows_counted")
        torch.cuda.synchronize()
        for k in ("ctl", "state", "ids", "tokens", "logprobs"):
            assert torch.equal(a[k], b[k]), (call, k)
        stamps.append((int(a["stamp"][0]), int(b["stamp"][0])))
    active = [int((ctl0[:, 0] >= 0).sum())]
    print(f"counted tail R {R} V {V}: stamps {stamps}, rows active at the start {active[0]}, at the end {int((b['ctl'][:, 0] >= 0).sum())}")
    assert [s >> 1 for _, s in stamps] == [1, 2, 3] and all(x == y for x, y in stamps)
    assert (stamps[2][1] & 1) == int(bool((b["ctl"][:, 0] < 0).all()))
    if R == 1:
        assert stamps == [(3, 3), (5, 5), (7, 7)]                      # its one row has a single pick: nobody is active from the first call on
    if R == 40:
        assert [s & 1 for _, s in stamps] == [0, 0, 0]                 # rows with five picks are still going
    assert count.tolist() == [-5, 3, -6]
    assert bool((b["tokens"] != -7).any()) and not torch.equal(b["state"], state0)          # the calls did pick
    # the stamp is optional, the counter is not
    _lib.check(lib.hirest_whisper_step_tail_rows_counted(logits.data_ptr(), V, R, V, count[1:].data_ptr(), ld, C.byref(params), b["ctl"].data_ptr(),
                                                         b["state"].data_ptr(), b["ids"].data_ptr(), b["tokens"].data_ptr(), None, None,
                                                         ops.stream_ptr()), "hirest_whisper_step_tail_rows_counted")
    torch.cuda.synchronize()
    assert count.tolist() == [-5, 4, -6] and int(b["stamp"][0]) == stamps[2][1]
    assert lib.hirest_whisper_step_tail_rows_counted(logits.data_ptr(), V, R, V, None, ld, C.byref(params), b["ctl"].data_ptr(), b["state"].data_ptr(),
                                                     b["ids"].data_ptr(), b["tokens"].data_ptr(), None, None, ops.stream_ptr()) == -1


# ---------------------------------------------------------------------------------------------------------------- the loop
_OWN = {}


def model(case, dev):
    """a model of this module's own (its weight preparation is dropped and rebuilt here), the case's audio states and fixture"""
    if case not in _OWN:
        _OWN[case] = S.model_for(case, dev)
    _, xa, z, _, _ = S.decoder(case, dev)
    return _OWN[case], xa, z


def long_model(dev):
    """a decoder with the released text context of 448, so that a prompt of 223 previous tokens exists: (model, xa [3, 70, 128])"""
    if "long" not in _OWN:
        cfg, eot, seed = dict(synth.WHISPER_DEC_LONG[0], max_target_positions=448), 100, 91
        enc = synth.whisper_encoder_state_dict(cfg, 73)
        sd = {**{"encoder." + k: v for k, v in enc.items()}, **synth.whisper_decoder_state_dict(cfg, seed, eot, 0.0)}
        _OWN["long"] = (whisper.Whisper(cfg, sd, synth.whisper_tokenizer(eot)).to(dev), synth.whisper_audio_states(cfg, 3, seed + 100).to(dev))
    return _OWN["long"]


def same_result(a, b):
    return (a.tokens, a.avg_logprob, a.no_speech_prob, a.temperature, a.text, a.compression_ratio, a.language) == \
           (b.tokens, b.avg_logprob, b.no_speech_prob, b.temperature, b.text, b.compression_ratio, b.language)


def delta(m, before):
    return {k: v - before[k] for k, v in m.graph_stats().items()}


def test_fails_without_the_feature():
    """what the tree before this option lacks: the keyword, the counted entry and the counters"""
    for fn in (whisper.decode, whisper.decode_many, whisper.transcribe, whisper.transcribe_many, whisper.Whisper.decode):
        assert inspect.signature(fn).parameters["graph"].default is None, fn
    assert hasattr(_lib.load(), "hirest_whisper_step_tail_rows_counted") and hasattr(whisper.Whisper, "graph_stats")


@pytest.mark.parametrize("case, window", [("p", 0), ("q", 0), ("q", 1)])
def test_greedy_decode_equals_eager(case, window, dev):
    m, xa, z = model(case, dev)
    for o in (O(temperature=0.0), O(temperature=0.0, prompt=z["prompt9"].tolist()), O(temperature=0.0, without_timestamps=True)):
        before = m.graph_stats()
        want = whisper.decode(m, xa[window], o)
        d = delta(m, before)
        assert d["captures"] == d["replays"] == 0 and d["eager_steps"] >= 1          # the option off: the loop of before
        got = whisper.decode(m, xa[window], o, graph=True)
        assert same_result(got, want), (o, got.tokens, want.tokens)
        assert torch.equal(got.audio_features, want.audio_features)
        assert m.decode(xa[window], o, graph=True).tokens == want.tokens
    if window == 0:
        assert want.tokens == z["greedy_01_tokens"].tolist()
    d = delta(m, before)
    assert d["eager_steps"] >= 3 and d["replays"] >= 1                 # an eager loop, then iteration 0 of two replayed ones


def test_sampled_decode_equals_eager(dev):
    m, xa, z = model("q", dev)
    for o in (O(temperature=0.4, best_of=5, seed=5), O(temperature=0.4, best_of=5, seed=6, prompt=z["prompt9"].tolist())):
        want, want_c = whisper.decode(m, xa[1], o, return_candidates=True)
        got, got_c = whisper.decode(m, xa[1], o, return_candidates=True, graph=True)
        assert same_result(got, want) and got_c == want_c and len(got_c) == 5
        assert len({tuple(t) for t, _ in got_c}) > 1                   # not five copies
    # a batch of windows: one replayed loop per window
    res = whisper.decode(m, xa, o, graph=True)
    assert all(same_result(a, b) for a, b in zip(res, whisper.decode(m, xa, o)))


def fill_arena(dec, R, n_windows, Tk):
    """the arena the next loop of this shape on the current stream will take, its self caches filled with the canary"""
    arena = whisper._decode_arena(dec, R, n_windows, Tk)
    for t in arena.self_k + arena.self_v:
        t.fill_(CANARY)
    return arena


def check_canaries(arena, m, opts, cands, steps):
    """past a row's last filled position the cache still holds the canary, in every layer; the positions up to it do not.  A row fills
    its prompt's positions and one more per pick after which it stayed active: every sampled token but the one that used its last step."""
    r = 0
    for o, cand, n_steps in zip(opts, cands, steps):
        T = len(whisper._initial_tokens(m.tokenizer, o, m.decoder.ctx)[0])
        for tokens, _ in cand:
            filled = T + len(tokens) - (1 if len(tokens) == n_steps else 0)
            for t in arena.self_k + arena.self_v:
                assert bool((t[r, filled:] == CANARY).all()), (r, T, len(tokens), filled)
                assert not bool((t[r, :filled] == CANARY).any()), (r, T, len(tokens), filled)
            r += 1
    assert r == arena.R


def test_decode_many_equals_eager_and_writes_no_position_past_a_row(dev):
    m, xa = long_model(dev)
    dec, tok = m.decoder, m.tokenizer
    text = synth.token_ids("graph.long.prompt", 300, 100, 7).tolist()
    opts = [O(temperature=0.0), O(temperature=0.4, best_of=3, seed=2, prompt=text[:260]), O(temperature=0.0, prompt=text[260:269])]
    lengths = [len(whisper._initial_tokens(tok, o, dec.ctx)[0]) for o in opts]
    assert dec.ctx == 448 and lengths[1] - lengths[0] == 224 and lengths[2] - lengths[0] == 10          # <|startofprev|> + 223 previous tokens
    # (1) the public call: one sample_len for all windows
    shared = [dataclasses.replace(o, sample_len=20) for o in opts]
    want, want_c = whisper.decode_many(m, xa, shared, return_candidates=True)
    arena = fill_arena(dec, 5, 3, int(xa.shape[1]))
    before = m.graph_stats()
    got, got_c = whisper.decode_many(m, xa, shared, return_candidates=True, graph=True)
    assert whisper._decode_arena(dec, 5, 3, int(xa.shape[1])) is arena and delta(m, before)["captures"] == 1
    assert got_c == want_c and all(same_result(a, b) for a, b in zip(got, want))
    check_canaries(arena, m, shared, got_c, [20] * 3)
    print(f"decode_many graph, sample_len 20: prompts {lengths}, sampled lengths {[[len(t) for t, _ in c] for c in got_c]}")
    # (2) a step budget per window — 1, 11 and 20: the first window ends at its first pick, the others in the second and third chunk —
    # as the plans of one loop; the yardstick is the eager decode() of each window with its own sample_len
    budgets = [1, 11, 20]
    own = [dataclasses.replace(o, sample_len=s) for o, s in zip(opts, budgets)]
    want = [whisper.decode(m, xa[w], o, return_candidates=True) for w, o in enumerate(own)]
    plans = []
    for o, s in zip(own, budgets):
        initial, sot_index = whisper._initial_tokens(tok, o, dec.ctx)
        plans.append((initial, sot_index, s, (o.best_of or 1) if o.temperature > 0 else 1))
    langs = [(None, None)] * 3
    eager, eager_c = whisper._decode_rows(m, xa, own, plans, langs)
    fill_arena(dec, 5, 3, int(xa.shape[1]))
    before = m.graph_stats()
    got, got_c = whisper._decode_rows(m, xa, own, plans, langs, graph=True)
    d = delta(m, before)
    assert d["captures"] == 0 and d["eager_steps"] == 1 and d["replays"] <= math.ceil(20 / whisper.DECODE_GRAPH_CHUNK) + 2
    assert got_c == eager_c and all(same_result(a, b) for a, b in zip(got, eager))
    for w in range(3):
        assert got_c[w] == want[w][1] and same_result(got[w], want[w][0]), w
    assert len(got_c[0][0][0]) <= 1
    check_canaries(arena, m, own, got_c, budgets)
    print(f"decode_many graph, budgets {budgets}: sampled lengths {[[len(t) for t, _ in c] for c in got_c]}, replays {d['replays']}")


@pytest.mark.parametrize("chunk, sample_len", [(8, 5), (8, 9), (2, 3), (8, 24), (4, 24), (16, 24)])
def test_loops_that_end_inside_a_chunk_and_at_its_edge(chunk, sample_len, dev, monkeypatch):
    """(8, 5): inside the first chunk.  (8, 9): iteration 0 and exactly one chunk.  (2, 3): CHUNK + 1 steps.  The others: the whole
    default budget, at the chunk lengths the measurements use."""
    m, xa, z = model("q", dev)
    monkeypatch.setattr(whisper, "DECODE_GRAPH_CHUNK", chunk)
    o = O(temperature=0.0, sample_len=sample_len)
    want = whisper.decode(m, xa[0], o)
    assert want.tokens == z["greedy_00_tokens"].tolist()[:sample_len] and len(want.tokens) == sample_len      # the budget ends it, not eot
    before = m.graph_stats()
    got = whisper.decode(m, xa[0], o, graph=True)
    d = delta(m, before)
    assert same_result(got, want)
    print(f"chunk {chunk}, {sample_len} steps: {d}")
    assert d["eager_steps"] == 1 and d["captures"] <= 1
    assert 1 <= d["replays"] <= math.ceil(sample_len / chunk) + 2
    assert 1 + d["replays"] * chunk >= sample_len                      # every tail the row needed was issued


def test_a_loop_that_eot_ends_wastes_at_most_two_chunks(dev):
    m, xa, z = model("p", dev)
    want = whisper.decode(m, xa[0], O(temperature=0.0))
    assert want.tokens == z["greedy_00_tokens"].tolist() and len(want.tokens) == 1          # two tails of a budget of 24
    before = m.graph_stats()
    got = whisper.decode(m, xa[0], O(temperature=0.0), graph=True)
    d = delta(m, before)
    assert same_result(got, want) and d["replays"] <= math.ceil(2 / whisper.DECODE_GRAPH_CHUNK) + 2, d


def test_arena_reuse_and_drop(dev):
    m, xa, z = model("q", dev)
    one, five = O(temperature=0.0), O(temperature=0.4, best_of=5, seed=5)
    want1, want5 = whisper.decode(m, xa[0], one), whisper.decode(m, xa[1], five, return_candidates=True)
    m.float()                                                          # (whatever arenas the tests before left: gone)
    before = m.graph_stats()
    whisper.decode(m, xa[0], one, graph=True)
    assert delta(m, before) == {"captures": 1, "replays": 3, "eager_steps": 1}          # 24 steps, none of them eot: iteration 0 and 3 chunks of 8
    before = m.graph_stats()
    assert same_result(whisper.decode(m, xa[0], one, graph=True), want1)
    assert same_result(whisper.decode(m, xa[1], O(temperature=0.0, prompt=z["prompt9"].tolist()), graph=True),
                       whisper.decode(m, xa[1], O(temperature=0.0, prompt=z["prompt9"].tolist())))
    assert delta(m, before)["captures"] == 0                           # the same R: the arena's graph, whatever window and prompt
    got5 = whisper.decode(m, xa[1], five, return_candidates=True, graph=True)
    assert delta(m, before)["captures"] == 1                           # another R captures once more ...
    assert same_result(got5[0], want5[0]) and got5[1] == want5[1]
    assert same_result(whisper.decode(m, xa[0], one, graph=True), want1) and delta(m, before)["captures"] == 1          # ... and keeps the first
    arenas = m.decoder._w()["decode_arenas"]
    assert len(arenas) >= 2
    for move in (lambda: m.to(dev), lambda: m.float()):                # any move or cast drops the weight preparation, the graphs with it
        move()
        assert m.decoder._cache is None
        before = m.graph_stats()
        assert same_result(whisper.decode(m, xa[0], one, graph=True), want1)
        assert delta(m, before)["captures"] == 1 and len(m.decoder._w()["decode_arenas"]) == 1
    # more shapes than arenas are kept: the least recently used goes, and a shape that comes back captures again
    for best_of in range(2, 2 + whisper.DECODE_ARENAS):
        whisper.decode(m, xa[0], O(temperature=0.4, best_of=best_of, seed=1), graph=True)
    assert len(m.decoder._w()["decode_arenas"]) == whisper.DECODE_ARENAS
    before = m.graph_stats()
    assert same_result(whisper.decode(m, xa[0], one, graph=True), want1) and delta(m, before)["captures"] == 1


def test_on_a_side_stream(dev):
    m, xa, z = model("q", dev)
    o = O(temperature=0.4, best_of=5, seed=5, prompt=z["prompt9"].tolist())
    want, want_c = whisper.decode(m, xa[1], o, return_candidates=True)
    whisper.decode(m, xa[1], o, graph=True)                            # the default stream's arena of this shape
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    before = m.graph_stats()
    with torch.cuda.stream(side):
        got, got_c = whisper.decode(m, xa[1], o, return_candidates=True, graph=True)
        again, again_c = whisper.decode(m, xa[1], o, return_candidates=True, graph=True)
    torch.cuda.synchronize()
    assert same_result(got, want) and got_c == want_c and same_result(again, want) and again_c == want_c
    assert delta(m, before)["captures"] == 1                           # the stream is part of the arena's key


def test_environment_turns_it_on(dev, monkeypatch):
    m, xa, _ = model("q", dev)
    want = whisper.decode(m, xa[0], O(temperature=0.0))
    monkeypatch.setenv("HIREST_WHISPER_GRAPH", "1")
    before = m.graph_stats()
    assert same_result(whisper.decode(m, xa[0], O(temperature=0.0)), want) and delta(m, before)["replays"] >= 1
    before = m.graph_stats()
    assert same_result(whisper.decode(m, xa[0], O(temperature=0.0), graph=False), want) and delta(m, before)["replays"] == 0


def test_graph_refuses_more_steps_than_its_tokens_hold(dev):
    m, xa, _ = model("q", dev)
    with pytest.raises(ValueError, match="n_text_ctx // 2"):
        whisper.decode(m, xa[0], O(temperature=0.0, sample_len=30), graph=True)


# ---------------------------------------------------------------------------------------------------------------- the loop state
def eager_loop_state(dev, monkeypatch):
    """``_decode_rows`` without the option over two windows of case p whose prompts differ in length, one greedy row and two sampled
    ones, three steps each -> (model, xa [2, 33, 128], the state the loop made, the prompts' lengths, what graph_stats moved by)"""
    m, _, _ = model("p", dev)
    m.float()                                                          # (whatever arenas the tests before left: gone)
    cfg, _, seed, _ = synth.WHISPER_DEC_CASES["p"]
    xa = synth.whisper_audio_states(cfg, 2, seed + 100).to(dev)
    opts = [O(temperature=0.0, sample_len=3), O(temperature=0.4, best_of=2, seed=3, sample_len=3, prompt=[5, 6, 7, 8, 9])]
    plans = []
    for o in opts:
        initial, sot_index = whisper._initial_tokens(m.tokenizer, o, m.decoder.ctx)
        plans.append((initial, sot_index, 3, (o.best_of or 1) if o.temperature > 0 else 1))
    made, init = [], whisper.DecodeState.__init__

    def spy(self, *a, **k):
        made.append(self)
        init(self, *a, **k)
    monkeypatch.setattr(whisper.DecodeState, "__init__", spy)
    before = m.graph_stats()
    results, cands = whisper._decode_rows(m, xa, opts, plans, [(None, None)] * 2)
    assert len(made) == 1 and [len(c) for c in cands] == [1, 2] and all(len(r.tokens) <= 3 for r in results)
    return m, xa, made[0], [len(p[0]) for p in plans], delta(m, before)


def test_eager_state_is_sized_by_its_loop(dev, monkeypatch):
    m, xa, state, lengths, d = eager_loop_state(dev, monkeypatch)
    dec = m.decoder
    assert lengths[1] - lengths[0] == 6 and max(lengths) + 3 < dec.ctx          # <|startofprev|> + 5 previous tokens
    assert state.R == 3 and state.T_max == max(lengths) + 3
    for t in state.self_k + state.self_v:
        assert t.shape == (3, max(lengths) + 3, dec.width)
    assert state.tokens.shape == (3, 3) and state.row_window.tolist() == [0, 1, 1]
    assert not dec._w().get("decode_arenas")                           # absent, or empty
    assert d["captures"] == d["replays"] == 0 and 1 <= d["eager_steps"] <= 3, d


def test_both_loops_run_on_one_state_class(dev, monkeypatch):
    m, xa, state, _, _ = eager_loop_state(dev, monkeypatch)
    dec = m.decoder
    arena = whisper._decode_arena(dec, 3, 2, int(xa.shape[1]))
    assert type(arena) is type(state) and isinstance(arena, whisper.KVCache)
    assert arena.T_max == dec.ctx and arena.tokens.shape == (3, dec.ctx // 2)
    for t in arena.self_k + arena.self_v:
        assert t.shape == (3, dec.ctx, dec.width)
    assert dec._w()["decode_arenas"] and whisper._decode_arena(dec, 3, 2, int(xa.shape[1])) is arena


def test_step_rows_method_equals_the_entry(dev):
    m, _, _ = model("p", dev)
    dec = m.decoder
    cfg, _, seed, _ = synth.WHISPER_DEC_CASES["p"]
    xa = synth.whisper_audio_states(cfg, 2, seed + 100).to(dev)
    T, positions = 4, (0, 2, -1)
    ctl = whisper.new_row_ctl([(p, 0, T, 0, 0, 0.0) for p in positions], dev)
    ids = torch.tensor([3, 17, 42], dtype=torch.int32, device=dev)

    def prepared():
        kc = whisper.KVCache(dec, xa, torch.tensor([0, 1, 1], dtype=torch.int32), T, per_row=True)
        for t in kc.self_k + kc.self_v + [kc.logits]:
            t.fill_(CANARY)
        return kc
    a, b = prepared(), prepared()
    assert dec.step_rows(ctl, ids, a) is a.logits
    _lib.check(_lib.load().hirest_whisper_decode_step_rows(C.byref(dec._w()["desc"]), 3, ctl.data_ptr(), ids.data_ptr(), b.k_ptrs, b.v_ptrs, b.T_max,
                                                           b.x_ptrs, b.n_windows, b.Tk, b.row_window.data_ptr(), b.logits.data_ptr(),
                                                           b.ws.data_ptr(), b.ws.numel(), ops.stream_ptr()), "hirest_whisper_decode_step_rows")
    torch.cuda.synchronize()
    assert torch.equal(a.logits, b.logits) and not bool((a.logits[:2] == CANARY).any())
    for x, y in zip(a.self_k + a.self_v, b.self_k + b.self_v):
        assert torch.equal(x, y)
        assert bool((x[2] == CANARY).all())                            # the inactive row's cache
        for r, p in enumerate(positions[:2]):                          # an active row wrote its own position and no other
            assert not bool((x[r, p] == CANARY).any())
            assert bool((x[r, :p] == CANARY).all()) and bool((x[r, p + 1:] == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------- transcribe
def test_transcribe_equals_eager(dev):
    """31 s of synthetic audio — two windows — through the case-p decoder behind the 1500-position encoder, with the temperature
    fallback, and the same again with word timestamps; transcribe_many over two files likewise"""
    m = S.model_for("p", dev, synth.WHISPER_E2E)
    audio = synth.audio_clip("mixed", 31 * 16000, 71)
    kw = dict(temperature=(0.0, 0.4), best_of=5)
    for extra in ({}, {"word_timestamps": True}):
        want = whisper.transcribe(m, audio, **kw, **extra)
        before = m.graph_stats()
        got = whisper.transcribe(m, audio, graph=True, **kw, **extra)
        d = delta(m, before)
        assert got == want and len({s["seek"] for s in got["segments"]}) >= 1 and d["replays"] >= 2, d
        print(f"transcribe graph {extra}: {len(got['segments'])} segments, seeks {sorted({s['seek'] for s in got['segments']})}, "
              f"temperatures {sorted({s['temperature'] for s in got['segments']})}, {d}")
    assert all("words" in s for s in got["segments"])
    short = synth.audio_clip("mixed", int(12.3 * 16000), 5)
    assert whisper.transcribe_many(m, [audio, short], files_in_flight=2, graph=True, **kw) == whisper.transcribe_many(m, [audio, short], files_in_flight=2, **kw)
    assert m.transcribe(short, graph=True, **kw) == whisper.transcribe(m, short, **kw)
