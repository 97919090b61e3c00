"""Windows of several files in one decoding loop: the per-row forms of the in-place self-attention and of the step tail,
decode_many() and transcribe_many().  Every comparison is equality with the single-window path — hirest_attention_f32_decode_inplace,
hirest_whisper_step_tail, decode(), transcribe() — which tests/test_gpu_whisper_dec.py pins to fp64 transformers: no tolerances here.
decode() runs the per-row loop too, one window at a time, so every decode() reference is also held equal to the lock-step loop over
TextDecoder.prefill / step (tests/_whisper_lockstep.py)."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

import test_gpu_whisper_dec as S
from _whisper_lockstep import lockstep_decode
from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

CANARY = S.CANARY


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- ragged attention
def test_decode_inplace_rows_equals_one_call_per_row(dev):
    lib = _lib.load()
    H, T_max = 2, 224
    D = 64 * H
    ts = [0, 1, -1, 63, 64, T_max, 65, 223]                            # an inactive row between the others, and one with a full cache
    R_ = len(ts)
    active = [r for r, t in enumerate(ts) if 0 <= t < T_max]
    assert len(active) == 6
    hist_k, hist_v = S.seeded("rows.k", (R_, T_max, D), 3, 1.5).to(dev), S.seeded("rows.v", (R_, T_max, D), 4, 1.0).to(dev)
    qkv = S.seeded("rows.qkv", (R_, 3 * D), 5, 3.0).to(dev)
    # one guard row in front of and one behind the call's rows, in the caches and in out
    ck = torch.full((R_ + 2, T_max, D), CANARY, dtype=torch.float32, device=dev)
    cv = torch.full((R_ + 2, T_max, D), CANARY, dtype=torch.float32, device=dev)
    for r in active:
        ck[r + 1, :ts[r]], cv[r + 1, :ts[r]] = hist_k[r, :ts[r]], hist_v[r, :ts[r]]
    want_k, want_v = ck.clone(), cv.clone()
    want = torch.full((R_ + 2, D), CANARY, dtype=torch.float32, device=dev)
    for r in active:                                                  # the yardstick: one scalar-position call per row, on that row alone
        q1 = qkv[r:r + 1].contiguous()
        _lib.check(lib.hirest_attention_f32_decode_inplace(q1.data_ptr(), 3 * D, want_k[r + 1].data_ptr(), want_v[r + 1].data_ptr(), D, T_max * D,
                                                           ts[r], T_max, q1.data_ptr() + 4 * D, q1.data_ptr() + 8 * D, 3 * D, want[r + 1].data_ptr(),
                                                           1, H, 0.125, 0.0, 0.0, ops.stream_ptr()), "hirest_attention_f32_decode_inplace")
    got = torch.full((R_ + 2, D), CANARY, dtype=torch.float32, device=dev)
    t_dev = torch.tensor(ts, dtype=torch.int32, device=dev)
    _lib.check(lib.hirest_attention_f32_decode_inplace_rows(qkv.data_ptr(), 3 * D, ck[1].data_ptr(), cv[1].data_ptr(), D, T_max * D, t_dev.data_ptr(),
                                                            T_max, qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, got[1].data_ptr(), R_, H,
                                                            0.125, 0.0, 0.0, ops.stream_ptr()), "hirest_attention_f32_decode_inplace_rows")
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(ck, want_k) and torch.equal(cv, want_v)
    for r in active:
        assert torch.equal(ck[r + 1, ts[r]], qkv[r, D:2 * D]) and torch.equal(cv[r + 1, ts[r]], qkv[r, 2 * D:]), r
    for r in [-1, R_] + [r for r in range(R_) if r not in active]:    # the guards and the inactive rows keep their sentinel everywhere
        assert bool((ck[r + 1] == CANARY).all()) and bool((cv[r + 1] == CANARY).all()) and bool((got[r + 1] == CANARY).all()), r
    assert lib.hirest_attention_f32_decode_inplace_rows(qkv.data_ptr(), 3 * D, ck[1].data_ptr(), cv[1].data_ptr(), D, T_max * D, None, T_max,
                                                        qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, got[1].data_ptr(), R_, H, 0.125, 0.0,
                                                        0.0, ops.stream_ptr()) == -1


# ---------------------------------------------------------------------------------------------------------------- ragged tail
def row_states(c, seqs, completed, sum0):
    st = torch.zeros((len(seqs), 8), dtype=torch.int32)
    for r, seq in enumerate(seqs):
        stamps = [t for t in seq if t >= c.timestamp_begin]
        st[r, :5] = torch.tensor([len(seq), seq[-1] if seq else -1, seq[-2] if len(seq) > 1 else -1, stamps[-1] if stamps else -1, int(completed[r])])
    st[:, 5] = torch.tensor(sum0, dtype=torch.float32).view(torch.int32)
    return st


def tail_rows_call(c, logits, rows, dev, call, ld_tokens=8):
    """one hirest_whisper_step_tail_rows call: rows = dicts of seq, sum0, position, step, max_steps, draw_row, seed, temperature"""
    lib = _lib.load()
    R_, V = logits.shape
    words = np.zeros((V + 31) // 32, dtype=np.uint32)
    for t in c.suppress:
        words[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    mask = torch.from_numpy(words.view(np.int32)).to(dev)
    p = _lib.WhisperTailParams()
    p.n_vocab, p.eot, p.no_speech, p.no_timestamps, p.timestamp_begin = V, c.eot, c.no_speech, c.no_timestamps, c.timestamp_begin
    p.max_initial_timestamp_index = -1 if c.max_initial_timestamp_index is None else c.max_initial_timestamp_index
    p.blank, p.suppress_blank, p.timestamp_rules, p.monotonic = c.blank, int(c.suppress_blank), int(c.timestamp_rules), int(c.monotonic)
    p.sample_begin, p.temperature, p.seed, p.serial = 5, 0.9, 1234, 77      # the per-call fields: this entry point must not look at them
    p.suppress_mask = mask.data_ptr()
    state = row_states(c, [r["seq"] for r in rows], [False] * R_, [r["sum0"] for r in rows]).to(dev)
    state0 = state.clone()
    ctl = whisper.new_row_ctl([(r["position"], r["step"], r["max_steps"], r["draw_row"], r["seed"], r["temperature"]) for r in rows], dev)
    ctl0 = ctl.clone()
    ids = torch.full((R_ + 1,), -7, dtype=torch.int32, device=dev)
    toks = torch.full((R_ + 1, ld_tokens), -7, dtype=torch.int32, device=dev)
    stamp = torch.zeros(1, dtype=torch.int32).pin_memory()
    x = logits.to(dev)
    _lib.check(lib.hirest_whisper_step_tail_rows(x.data_ptr(), V, R_, V, call, ld_tokens, C.byref(p), ctl.data_ptr(), state.data_ptr(), ids.data_ptr(),
                                                 toks.data_ptr(), None, stamp.data_ptr(), ops.stream_ptr()), "hirest_whisper_step_tail_rows")
    torch.cuda.synchronize()
    assert int(ids[R_]) == -7 and bool((toks[R_] == -7).all())
    return {"state": state.cpu(), "state0": state0.cpu(), "ctl": ctl.cpu(), "ctl0": ctl0.cpu(), "ids": ids[:R_].cpu().numpy(),
            "tokens": toks[:R_].cpu().numpy(), "stamp": int(stamp[0])}


def check_rows_against_single_calls(c, logits, rows, got, dev):
    for r, row in enumerate(rows):
        st, ctl = got["state"][r], got["ctl"][r]
        if row["position"] < 0:                                       # an inactive row changes nothing
            assert torch.equal(st, got["state0"][r]) and torch.equal(ctl, got["ctl0"][r]) and got["ids"][r] == -7
            assert (got["tokens"][r] == -7).all()
            continue
        # the yardstick: the single-window call with the row's parameters, in a call large enough that the row sits at index draw_row
        n, g = row["draw_row"] + 1, row["draw_row"]
        ref = S.tail_call(c, logits[r:r + 1].expand(n, -1).contiguous(), [row["seq"]] * n, [False] * n, [row["sum0"]] * n, dev,
                          temperature=row["temperature"], seed=row["seed"], serial=row["step"], step=row["step"], want_logprobs=False)
        pick = int(ref["ids"][g])
        assert got["ids"][r] == pick and got["tokens"][r, row["step"]] == pick, (r, got["ids"][r], pick)
        assert (np.delete(got["tokens"][r], row["step"]) == -7).all()
        assert st[:5].tolist() == ref["state"][g].tolist(), r
        f = st[5:8].view(torch.float32).numpy()
        assert f[0] == ref["sum"][g] and f[1] == ref["no_speech"][g] and f[2] == ref["last_lp"][g], (r, f, ref["sum"][g])
        ends = pick == c.eot or row["step"] + 1 == row["max_steps"]
        assert ctl[:4].tolist() == [-1 if ends else row["position"] + 1, row["step"] + 1, row["max_steps"], row["draw_row"]], (r, ctl)
        assert torch.equal(ctl[4:], got["ctl0"][r][4:])
        assert int(st[4]) == int(pick == c.eot)                       # out of room is not completed


@pytest.mark.parametrize("V", [200, 51864])
def test_tail_rows_equal_one_call_per_row(V, dev):
    c = S.consts_for(V)
    hist = S.rule_histories(c)
    row = lambda name, sum0, position, step, max_steps, draw_row, seed, temperature: dict(
        seq=hist[name], sum0=sum0, position=position, step=step, max_steps=max_steps, draw_row=draw_row, seed=seed, temperature=temperature)
    rows = [row("after_closed_pair", -0.5, 30, 4, 24, 3, 21, 0.4),
            row("text", -1.25, 7, 2, 3, 1, 0xFFFFFFF0, 0.8),           # its last pick: goes inactive without completing
            row("text", -2.0, 11, 3, 24, 4, 9, 0.0)]                   # greedy, and its logits below make it pick eot
    if V == 200:
        rows += [row("first", 0.0, 0, 0, 24, 0, 5, 0.0), row("text", -3.0, -1, 1, 24, 2, 3, 0.4),       # an inactive row between the others
                 row("after_text_ts", -0.75, 46, 5, 24, 2, 21, 0.8), row("last_ts_at_max_open", -0.1, 5, 1, 2, 0, 6, 0.4)]
    logits = S.seeded("tailrows.logits", (len(rows), V), V + 2, 3.0)
    logits[1, c.eot] = -30.0
    logits[2, c.eot] = 40.0
    got = tail_rows_call(c, logits, rows, dev, call=6)
    check_rows_against_single_calls(c, logits, rows, got, dev)
    assert got["ctl"][1, 0] == -1 and got["state"][1, 4] == 0 and got["ids"][1] != c.eot          # out of room, not completed, no eot written
    assert got["ctl"][2, 0] == -1 and got["state"][2, 4] == 1 and got["ids"][2] == c.eot
    assert got["ctl"][0, 0] == 31
    assert got["stamp"] == (7 << 1) | 0                               # row 0 is still active
    # the two rows that end, alone and with an inactive one: nobody is active afterwards, and two runs give the same bits
    ending = [rows[1], rows[2], dict(rows[0], position=-1)]
    done = tail_rows_call(c, logits[[1, 2, 0]], ending, dev, call=2)
    check_rows_against_single_calls(c, logits[[1, 2, 0]], ending, done, dev)
    assert done["stamp"] == (3 << 1) | 1
    assert torch.equal(done["state"][:2], got["state"][1:3]) and torch.equal(done["ctl"][:2], got["ctl"][1:3])
    # a further call on rows that are all inactive writes nothing but the stamp
    idle = tail_rows_call(c, logits[:2], [dict(rows[0], position=-1), dict(rows[1], position=-5)], dev, call=9)
    assert torch.equal(idle["state"], idle["state0"]) and torch.equal(idle["ctl"], idle["ctl0"]) and (idle["tokens"] == -7).all()
    assert idle["stamp"] == (10 << 1) | 1
    assert _lib.load().hirest_whisper_step_tail_rows(None, 0, 1, 4, 0, 8, None, None, None, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------- decode_many
def model(case, dev):
    if case not in S._MODELS:
        S._MODELS[case] = S.model_for(case, dev)
    return S._MODELS[case]


def same_result(a, b):
    return (a.tokens, a.avg_logprob, a.no_speech_prob, a.temperature, a.text, a.compression_ratio) == \
           (b.tokens, b.avg_logprob, b.no_speech_prob, b.temperature, b.text, b.compression_ratio)


def test_decode_many_equals_decode(dev, monkeypatch):
    m = model("q", dev)
    _, xa, z, _, _ = S.decoder("q", dev)
    prompt9 = z["prompt9"].tolist()
    prompt23 = (prompt9 * 3)[:23]                                      # 25 initial tokens + 24 to sample > 48 positions: the context cuts max_steps
    assert m.decoder.ctx == 48 and len(whisper._initial_tokens(m.tokenizer, whisper.DecodingOptions(prompt=prompt23), 48)[0]) == 25
    windows = [xa[0], xa[1], xa[0]]                                    # case q's two windows and the first again
    opts = [whisper.DecodingOptions(temperature=0.0), whisper.DecodingOptions(temperature=0.4, best_of=5, seed=5, prompt=prompt23),
            whisper.DecodingOptions(temperature=0.0, prompt=prompt9)]
    want = [whisper.decode(m, w, o, return_candidates=True) for w, o in zip(windows, opts)]
    assert len(want[1][1]) == 5 and max(len(t) for t, _ in want[1][1]) <= 23
    for (res, cands), w, o in zip(want, windows, opts):               # the per-row loop of one window against the lock-step loop
        assert (cands, res.no_speech_prob) == lockstep_decode(m, w, o)
    assert want[0][0].tokens == z["greedy_00_tokens"].tolist() and want[2][0].tokens == z["greedy_10_tokens"].tolist()
    for order in ([0, 1, 2], [2, 1, 0], [0, 1, 2]):                    # as given, reversed, and a second run
        res, cands = whisper.decode_many(m, [windows[i] for i in order], [opts[i] for i in order], return_candidates=True)
        assert len(res) == len(cands) == 3
        for k, i in enumerate(order):
            assert same_result(res[k], want[i][0]), (order, i, res[k].tokens, want[i][0].tokens)
            assert cands[k] == want[i][1], (order, i)
            assert torch.equal(res[k].audio_features, windows[i])
    # one DecodingOptions for all windows, as a tensor of windows
    both = whisper.decode_many(m, xa, opts[0])
    assert same_result(both[0], want[0][0]) and same_result(both[1], whisper.decode(m, xa[1], opts[0]))
    # past the row limit of one loop the windows go through consecutive loops: 1 + 5 rows, then 1, and 5 rows alone when nothing else fits
    for limit in (6, 3):
        monkeypatch.setattr(whisper, "_ROWS_PER_CALL", limit)
        res, cands = whisper.decode_many(m, windows, opts, return_candidates=True)
        assert all(same_result(res[i], want[i][0]) and cands[i] == want[i][1] for i in range(3)), limit


def test_decode_of_a_batch_equals_decode_of_each_window(dev):
    m = model("q", dev)
    _, xa, z, _, _ = S.decoder("q", dev)
    o = whisper.DecodingOptions(temperature=0.4, best_of=5, seed=5, prompt=z["prompt9"].tolist())
    res, cands = whisper.decode(m, xa, o, return_candidates=True)
    assert isinstance(res, list) and len(res) == len(cands) == xa.shape[0] == 2
    for w in range(2):
        one, one_c = whisper.decode(m, xa[w], o, return_candidates=True)
        assert same_result(res[w], one) and cands[w] == one_c and torch.equal(res[w].audio_features, xa[w])
    assert all(same_result(a, b) for a, b in zip(whisper.decode(m, xa, o), res))


def test_decode_many_of_one_window_equals_decode(dev):
    m = model("p", dev)
    _, xa, z, _, _ = S.decoder("p", dev)
    for o in (whisper.DecodingOptions(temperature=0.0), whisper.DecodingOptions(temperature=0.4, best_of=5, seed=5, prompt=z["prompt9"].tolist())):
        want, want_c = whisper.decode(m, xa[0], o, return_candidates=True)
        assert (want_c, want.no_speech_prob) == lockstep_decode(m, xa[0], o)
        (got,), (got_c,) = whisper.decode_many(m, xa[:1], [o], return_candidates=True)
        assert same_result(got, want) and got_c == want_c
    assert whisper.decode(m, xa[0], whisper.DecodingOptions(temperature=0.0)).tokens == z["greedy_00_tokens"].tolist()


def test_decode_many_refuses_options_that_must_be_shared(dev):
    m = model("p", dev)
    _, xa, _, _, _ = S.decoder("p", dev)
    with pytest.raises(ValueError, match="without_timestamps"):
        whisper.decode_many(m, [xa[0], xa[0]], [whisper.DecodingOptions(), whisper.DecodingOptions(without_timestamps=True)])
    with pytest.raises(ValueError, match="2 DecodingOptions for 1 windows"):
        whisper.decode_many(m, xa[:1], [whisper.DecodingOptions()] * 2)


# ---------------------------------------------------------------------------------------------------------------- transcribe_many
_E2E = {}


def e2e(dev, tmp_path_factory):
    """the model behind the 1500-position encoder, three inputs of about 12 s, 31 s and 65 s (the second as a .wav file) and transcribe() of
    each: built once"""
    if not _E2E:
        m = S.model_for("p", dev, synth.WHISPER_E2E)
        clips = [synth.audio_clip("mixed", int(s * 16000), seed) for s, seed in ((12.3, 5), (31.0, 71), (65.2, 9))]
        path = str(tmp_path_factory.mktemp("many") / "clip.wav")
        with wave.open(path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(clips[1], -1, 1 - 1 / 32768) * 32768).astype("<i2").tobytes())
        audios = [clips[0], path, clips[2]]
        kw = dict(temperature=(0.0, 0.4), best_of=5)
        _E2E.update(model=m, audios=audios, kw=kw, want=[whisper.transcribe(m, a, **kw) for a in audios])
    return _E2E


@pytest.mark.parametrize("files_in_flight", [1, 2, 3])
def test_transcribe_many_equals_transcribe(files_in_flight, dev, tmp_path_factory):
    e = e2e(dev, tmp_path_factory)
    got = whisper.transcribe_many(e["model"], e["audios"], files_in_flight=files_in_flight, **e["kw"])
    assert len(got) == 3
    keys = ("id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob")
    for g, w in zip(got, e["want"]):
        assert g["text"] == w["text"] and g["language"] == w["language"] and len(g["segments"]) == len(w["segments"])
        for a, b in zip(g["segments"], w["segments"]):
            assert [a[k] for k in keys] == [b[k] for k in keys], (files_in_flight, a, b)
    print(f"transcribe_many, {files_in_flight} in flight: segments per file {[len(g['segments']) for g in got]}, temperatures "
          f"{sorted({s['temperature'] for g in got for s in g['segments']})}")
    assert sum(len(g["segments"]) for g in got) > 0
