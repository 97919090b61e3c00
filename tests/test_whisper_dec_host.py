"""Whisper text decoder, the host side: tokenizer, options, transcribe()'s seek / segment / fallback logic on scripted decode results, .srt
writing, the numpy restatement of the tail's rules against transformers' processors, and the ABI of the new entry points."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch

import _whisper_dec_ref as R
from hirest_amd import _lib, dataset, synth, whisper
from hirest_amd.bytebpe import ByteBPETokenizer, bytes_to_unicode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("hirest_attention_f32_decode_inplace", "hirest_attention_f32_cross_decode_workspace_bytes", "hirest_attention_f32_cross_decode",
               "hirest_whisper_step_tail", "hirest_whisper_gumbel_bits", "hirest_whisper_step_workspace_bytes", "hirest_whisper_decode_step")


def test_new_entries_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hirest_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hirest_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.hirest_abi_version() == 4
    assert "whisper_dec.hip" in __import__("hirest_amd.build", fromlist=["SOURCES"]).SOURCES
    # argument checks that need no GPU
    assert lib.hirest_attention_f32_cross_decode_workspace_bytes(5, 12, 1500) == 5 * 12 * 24 * 68 * 4
    assert lib.hirest_attention_f32_cross_decode_workspace_bytes(5, 12, 1500) == lib.hirest_attention_f32_cross_decode_workspace_bytes(5, 12, 1473)
    assert lib.hirest_attention_f32_cross_decode(None, 0, None, 0, 0, 1, 1, None, None, 0, 1, 1, 1.0, None, 0, None) == -1
    assert lib.hirest_whisper_step_tail(None, 0, 1, 4, 0, 0, None, None, None, None, None, None, None) == -1


def test_bytebpe_decode_round_trip():
    table = bytes_to_unicode()
    vocab = {c: i for i, c in enumerate(table.values())}
    for t in ("<s>", "</s>", "<pad>"):
        vocab[t] = len(vocab)
    vocab["th"] = len(vocab)
    tok = ByteBPETokenizer(vocab, ["t h"])
    for text in ("the thing", "héllo wörld ♪ 「x」", "  spaces\n\ttabs"):
        ids = tok.tokenize_ids(text)
        assert tok.decode(ids) == text
    assert vocab["th"] in tok.tokenize_ids("the")


@pytest.fixture(scope="module")
def tok():
    return synth.whisper_tokenizer(50256)


def test_tokenizer_specials_and_round_trip(tok):
    sp = synth.whisper_special_tokens(50256)
    assert (tok.eot, tok.sot, tok.sot_prev, tok.no_speech, tok.no_timestamps, tok.timestamp_begin) == (50256, 50257, 50360, 50361, 50362, 50363)
    assert tok.sot_sequence == (50257,)
    assert sp["<|translate|>"] == 50357 and tok.transcribe == 50358 and tok.sot_lm == 50359
    text = " the thing in there — naïve"
    ids = tok.encode(text)
    assert all(0 <= i < 50256 for i in ids) and tok.decode(ids) == text
    assert len(tok.encode(" the")) == 1                               # merged down to one symbol
    stamped = [tok.timestamp_begin] + tok.encode(" the") + [tok.timestamp_begin + 54, tok.eot]
    assert tok.decode(stamped) == " the<|endoftext|>"
    assert tok.decode_with_timestamps(stamped) == "<|0.00|> the<|1.08|><|endoftext|>"
    ml = whisper.Tokenizer(*synth.whisper_vocab(50256), {**sp, "<|en|>": 50259}, language="en", task="transcribe")
    assert ml.sot_sequence == (50257, 50259, 50358)
    with pytest.raises(ValueError):
        whisper.Tokenizer(*synth.whisper_vocab(50256), {"<|endoftext|>": 50256})


def test_non_speech_tokens(tok):
    ns = tok.non_speech_tokens
    assert list(ns) == sorted(set(ns))
    for sym in "\"#()*+/:;<=>@[\\]^_`{|}~":
        assert tok.encode(sym)[0] in ns, sym
    assert tok.encode(" -")[0] in ns and tok.encode(" '")[0] in ns and len(tok.encode(" -")) == 1
    assert tok.encode("♪")[0] in ns                                   # a musical symbol: its first byte's token even though it takes three
    for keep in ("a", " the", ".", ",", "-", "'", "!", "?"):
        assert tok.encode(keep)[0] not in ns, keep
    assert tok.eot not in ns
    small = synth.whisper_tokenizer(100)                              # a reduced vocabulary: symbols it cannot spell are skipped
    assert small.eot not in small.non_speech_tokens and small.encode("(")[0] in small.non_speech_tokens


def test_decoding_options():
    with pytest.raises(NotImplementedError):
        whisper.DecodingOptions(beam_size=5)
    with pytest.raises(NotImplementedError):
        whisper.DecodingOptions(patience=1.0)
    with pytest.raises(ValueError):
        whisper.DecodingOptions(temperature=0.0, best_of=5)
    o = whisper.DecodingOptions(temperature=0.15, best_of=5, fp16=True)
    assert (o.suppress_tokens, o.suppress_blank, o.without_timestamps, o.max_initial_timestamp, o.prefix, o.sample_len) == ("-1", True, False, 1.0, None, None)
    r = whisper.DecodingResult(tokens=[1], text="x", avg_logprob=-0.5, no_speech_prob=0.1, temperature=0.0, compression_ratio=1.0)
    assert r.audio_features is None and r.language == "en"


def test_load_model_refuses_names(tmp_path):
    with pytest.raises(FileNotFoundError, match="not resolved and nothing is downloaded"):
        whisper.load_model("small.en")


def test_format_timestamp_and_write_srt_round_trip():
    assert whisper.format_timestamp(0.0) == "00:00.000"
    assert whisper.format_timestamp(3661.0006, always_include_hours=True, decimal_marker=",") == "01:01:01,001"
    assert whisper.utils.format_timestamp(59.9996) == "01:00.000"
    segs = [{"start": 0.0, "end": 2.5, "text": " first line"}, {"start": 2.5, "end": 61.25, "text": " a --> b"},
            {"start": 3599.98, "end": 3600.5, "text": " third"}]
    f = io.StringIO()
    whisper.utils.write_srt(segs, file=f)
    text = f.getvalue()
    assert text.startswith("1\n00:00:00,000 --> 00:00:02,500\nfirst line\n\n2\n00:00:02,500 --> 00:01:01,250\na -> b\n\n3\n")
    assert dataset.read_srt_spans(text) == [(0, 2), (2, 61), (3599, 3600)]


# ---------------------------------------------------------------------------------------------------------------------------------
# transcribe() on scripted decode results
# ---------------------------------------------------------------------------------------------------------------------------------

def _stub_model():
    return types.SimpleNamespace(dims={"n_mels": 80, "n_audio_ctx": 1500}, is_multilingual=False, device=torch.device("cpu"), tokenizer=None)


def _run(monkeypatch, tok, script, frames, **kw):
    """transcribe() over a zero spectrogram of ``frames`` content frames with decode() replaced by the script; returns the result and the
    (seek of the window, options) of every decode call"""
    calls, it = [], iter(script)

    def fake_decode(model, segment, options):
        assert tuple(segment.shape) == (80, 3000)
        calls.append((float(segment[0, 0]), options))
        return next(it)
    monkeypatch.setattr(whisper, "decode", fake_decode)
    mel = torch.zeros((80, frames + 3000))
    mel[0] = torch.arange(frames + 3000, dtype=torch.float32)          # row 0 carries the frame number: the stub sees where a window starts
    out = whisper.transcribe(_stub_model(), mel, tokenizer=tok, **kw)
    assert next(it, None) is None, "transcribe() made fewer decode calls than scripted"
    return out, calls


def _res(tok, tokens, temperature=0.0, avg_logprob=-0.2, no_speech_prob=0.01, compression_ratio=1.2):
    return whisper.DecodingResult(tokens=list(tokens), text=tok.decode(tokens), avg_logprob=avg_logprob, no_speech_prob=no_speech_prob,
                                  temperature=temperature, compression_ratio=compression_ratio)


def test_transcribe_two_closed_pairs_then_trailing_single(monkeypatch, tok):
    tb, a, b, c = tok.timestamp_begin, tok.encode(" the"), tok.encode(" thing"), tok.encode(" in")
    first = [tb] + a + [tb + 100, tb + 100] + b + [tb + 250, tb + 250]             # two closed pairs; the open third one is dropped
    second = [tb] + c + [tb + 50, tb + 50] + a + [tb + 120]                        # a pair, then text with a single timestamp at the end
    out, calls = _run(monkeypatch, tok, [_res(tok, first), _res(tok, second)], frames=3500, temperature=(0.0, 0.2), best_of=5)
    # window 1 ends at its last closed pair: 250 * 0.02 s = 5 s = frame 500; window 2 (3000 frames from there, all content) ends by a single
    # timestamp, so the whole window is consumed
    assert [c[0] for c in calls] == [0.0, 500.0]
    want = [(0, 0, 0.0, 2.0, " the", [tb] + a + [tb + 100]), (1, 0, 2.0, 5.0, " thing", [tb + 100] + b + [tb + 250]),
            (2, 500, 5.0, 6.0, " in", [tb] + c + [tb + 50]), (3, 500, 6.0, 7.4, " the", [tb + 50] + a + [tb + 120])]
    got = [(s["id"], s["seek"], s["start"], s["end"], s["text"], s["tokens"]) for s in out["segments"]]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:2] == w[:2] and g[4:] == w[4:] and g[2] == pytest.approx(w[2]) and g[3] == pytest.approx(w[3]), (g, w)
    assert out["text"] == " the thing in the" and out["language"] == "en"
    assert set(out["segments"][0]) == {"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}
    # greedy first: beam options are only dropped above temperature 0, best_of only at 0 — and beam search is not built
    assert calls[0][1].temperature == 0.0 and calls[0][1].best_of is None
    # the second window is conditioned on the first window's tokens
    assert calls[0][1].prompt == [] and calls[1][1].prompt == [tb] + a + [tb + 100] + [tb + 100] + b + [tb + 250]


def test_transcribe_greedy_with_beam_size_raises(monkeypatch, tok):
    with pytest.raises(NotImplementedError):
        _run(monkeypatch, tok, [], frames=100, temperature=0.0, beam_size=5)


def test_transcribe_no_timestamps_at_all(monkeypatch, tok):
    a = tok.encode(" the thing")
    out, calls = _run(monkeypatch, tok, [_res(tok, a), _res(tok, a)], frames=4000, temperature=0.0)
    assert [c[0] for c in calls] == [0.0, 3000.0]
    segs = out["segments"]
    assert [(s["start"], s["end"], s["seek"]) for s in segs] == [(0.0, 30.0, 0), (30.0, 40.0, 3000)]        # whole windows; the last has 1000 frames
    assert [s["text"] for s in segs] == [" the thing"] * 2


def test_transcribe_fallback_and_prompt_reset(monkeypatch, tok):
    tb, a = tok.timestamp_begin, tok.encode(" the")
    good = [tb] + a + [tb + 1500]
    script = [_res(tok, good, 0.15, compression_ratio=3.0),                      # too repetitive -> retry
              _res(tok, good, 0.35, avg_logprob=-1.5),                           # too unlikely -> retry
              _res(tok, good, 0.55),                                             # accepted; above 0.5: the next window gets no prompt
              _res(tok, good, 0.15)]
    out, calls = _run(monkeypatch, tok, script, frames=6000, temperature=(0.15, 0.35, 0.55, 0.75), best_of=5, beam_size=5, patience=1.0)
    assert [c[1].temperature for c in calls] == [0.15, 0.35, 0.55, 0.15]
    assert all(c[1].best_of == 5 and c[1].beam_size is None for c in calls)
    assert [c[0] for c in calls] == [0.0, 0.0, 0.0, 3000.0]
    assert calls[3][1].prompt == []
    assert [s["temperature"] for s in out["segments"]] == [0.55, 0.15]
    assert [(s["start"], s["end"]) for s in out["segments"]] == [(0.0, 30.0), (30.0, 60.0)]


def test_transcribe_skips_no_speech(monkeypatch, tok):
    tb, a = tok.timestamp_begin, tok.encode(" the")
    silent = _res(tok, [tb] + a + [tb + 10], avg_logprob=-1.2, no_speech_prob=0.9)
    unsure = _res(tok, [tb] + a + [tb + 10], avg_logprob=-0.3, no_speech_prob=0.9)        # probably speech after all: kept
    out, calls = _run(monkeypatch, tok, [silent, unsure], frames=6000, temperature=0.0, logprob_threshold=None)
    # without a log-probability threshold there is no fallback and the no-speech test alone decides
    assert [c[0] for c in calls] == [0.0, 3000.0] and out["segments"] == []
    out, calls = _run(monkeypatch, tok, [silent, silent, unsure], frames=6000, temperature=(0.0, 0.2))
    # window 1: both temperatures fall under the log-probability threshold, the result stays silent and is skipped; window 2 is kept
    assert [c[0] for c in calls] == [0.0, 0.0, 3000.0]
    assert [(s["seek"], s["start"], s["end"]) for s in out["segments"]] == [(3000, 30.0, 30.2)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the restated rules against transformers' processors
# ---------------------------------------------------------------------------------------------------------------------------------

def _legal_history(rng, c, n):
    """a random sequence of n sampled tokens that the rules themselves allow"""
    seq = []
    for _ in range(n):
        s = R.suppressed_before_lse(c, seq, c.n_vocab)
        s[c.eot] = True
        seq.append(int(rng.choice(np.flatnonzero(~s))))
    return seq


def test_tail_rules_equal_transformers_processors():
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(5)
    V, eot = 200, 100
    sp = synth.whisper_special_tokens(eot)
    nts = sp["<|notimestamps|>"]
    c = R.Consts(V, eot, sp["<|nospeech|>"], nts, nts + 1, 9, blank=3, suppress=[5, 17, 60, sp["<|startoftranscript|>"], sp["<|nospeech|>"]])
    begin = 4
    gc = types.SimpleNamespace(no_timestamps_token_id=nts, eos_token_id=eot, bos_token_id=eot, max_initial_timestamp_index=9)
    procs = [lp.SuppressTokensAtBeginLogitsProcessor([c.blank, eot], begin), lp.SuppressTokensLogitsProcessor(c.suppress),
             lp.WhisperTimeStampLogitsProcessor(gc, begin)]
    fired = 0
    for trial in range(300):
        n = int(rng.integers(0, 12))
        seq = _legal_history(rng, c, n)
        logits = rng.normal(0.0, 2.0, V)
        if trial % 3 == 0:
            logits[c.timestamp_begin:] += 2.0                        # makes the log-sum-exp rule fire on a good share of the trials
        ids = torch.tensor([[7, 8, 9, sp["<|startoftranscript|>"]] + seq])
        row = torch.from_numpy(logits)[None]
        for pr in procs:
            row = pr(ids, row)
        want = torch.isinf(row[0]).numpy()
        got = R.tail_row(c, logits, seq)
        assert np.array_equal(got["suppressed"], want), (trial, seq, np.flatnonzero(got["suppressed"] != want))
        fired += got["lse_gap"] is not None and got["lse_gap"] > 0
        assert got["pick"] == int(row[0].argmax())
        assert got["logprob"] == pytest.approx(float(torch.log_softmax(row[0], -1)[got["pick"]]), abs=1e-12)
        assert R.grammar_ok(c, seq)
    assert 30 < fired < 270
    assert not R.grammar_ok(c, [c.timestamp_begin, 1, c.timestamp_begin + 5, 2])              # an unpaired timestamp inside
    assert not R.grammar_ok(c, [c.timestamp_begin + 4, 1, c.timestamp_begin + 3])             # a decreasing one
    assert not R.grammar_ok(c, [1, 2])                                                        # no opening timestamp


def test_generator_restatement_is_pinned():
    bits = R.draw_bits(7, 3, 2, 4)
    assert bits.tolist() == [[7766746, 3210143, 3514999, 6106043], [2469677, 16020399, 3909363, 5066730]]
    b = R.draw_bits(11, 0, 64, 4096)
    assert b.max() < (1 << 24) and abs(float(b.mean()) / (1 << 24) - 0.5) < 0.002
    assert not np.array_equal(R.draw_bits(1, 2, 1, 64), R.draw_bits(2, 1, 1, 64))             # seed and serial do not commute


def test_decoder_tables_and_synth_cases():
    for case, (cfg, eot, seed, windows) in synth.WHISPER_DEC_CASES.items():
        sd = synth.whisper_decoder_state_dict(cfg, seed, eot, synth.WHISPER_DEC_EOT_BIAS[case]) if case != "r" else None
        if sd is None:
            continue
        dec = whisper.TextDecoder(cfg, sd)
        assert (dec.vocab, dec.width, dec.heads, dec.layers, dec.ctx) == (cfg["vocab_size"], cfg["d_model"], cfg["decoder_attention_heads"],
                                                                         cfg["decoder_layers"], cfg["max_target_positions"])
        # the OpenAI schema of the same weights gives the same parameters
        openai = {"decoder." + k.replace("/", "."): v for k, v in dec._parameters.items()}
        dims = {"n_vocab": dec.vocab, "n_text_ctx": dec.ctx, "n_text_state": dec.width, "n_text_head": dec.heads, "n_text_layer": dec.layers}
        again = whisper.TextDecoder(dims, openai)
        assert all(torch.equal(v, again._parameters[k]) for k, v in dec._parameters.items())
        with pytest.raises(RuntimeError, match="MI355X only"):
            dec(torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, cfg["max_source_positions"], dec.width)))
    # the encoder's table is untouched by the decoder's: an encoder still loads from a full checkpoint
    enc_sd = synth.whisper_encoder_state_dict(synth.WHISPER_DEC_P, 3)
    full = {**{"encoder." + k: v for k, v in enc_sd.items()}, **synth.whisper_decoder_state_dict(synth.WHISPER_DEC_P, 81)}
    model = whisper.Whisper(synth.WHISPER_DEC_P, full)
    assert model.dims["n_vocab"] == 200 and model.dims["n_audio_ctx"] == 33 and not model.is_multilingual


@pytest.mark.parametrize("case", synth.WHISPER_DEC_WIDTH_CASES)
def test_width_fixtures_agree_with_synth(case):
    cfg, eot, seed, windows = synth.WHISPER_DEC_CASES[case]
    path = os.path.join(REPO, "tests", "golden", f"whisper_dec_{case}.npz")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(REPO, "tests", "golden", "whisper_enc_c.npz"))
    z = np.load(path)
    T = 6
    assert z["tokens"].shape == (windows, T) and z["tokens"].dtype == np.int32
    assert z["hidden64"].shape == (windows, T, cfg["d_model"]) and z["hidden64"].dtype == np.float64 and np.isfinite(z["hidden64"]).all()
    assert 0 < float(z["err32"]) < 1e-3
    sp = synth.whisper_special_tokens(eot)
    assert (z["tokens"][:, 0] == sp["<|startoftranscript|>"]).all() and (z["tokens"][:, 1:] >= 0).all() and (z["tokens"][:, 1:] < eot).all()
    text = synth.token_ids(f"whisper.dec.{case}", windows * T, eot, seed).reshape(windows, T)
    assert np.array_equal(z["tokens"][:, 1:], text[:, 1:])
    assert cfg["d_model"] == 64 * cfg["decoder_attention_heads"] and cfg["max_source_positions"] == 70 and cfg["decoder_layers"] == 1
    assert T <= cfg["max_target_positions"]
    if case != "s":
        assert set(z.files) == {"tokens", "hidden64", "err32"}
        return
    # small.en's width with an LM head of at least 8192 columns, a multiple of 4; the special tokens and 188 timestamps fit behind eot
    assert cfg["vocab_size"] >= 8192 and cfg["vocab_size"] % 4 == 0 and windows == 3
    tok = synth.whisper_tokenizer(eot)
    k = synth.whisper_tail_consts(cfg, eot)
    assert eot < tok.sot < tok.no_timestamps < tok.timestamp_begin < cfg["vocab_size"] and k["max_initial_timestamp_index"] == 2
    assert tok.timestamp_begin + k["max_initial_timestamp_index"] < cfg["vocab_size"] and all(0 <= t < cfg["vocab_size"] for t in k["suppress"])
    greedy, (avg, nsp, err32, margin) = z["greedy_00_tokens"].tolist(), z["greedy_00_stats"]
    assert 4 <= len(greedy) < cfg["max_target_positions"] // 2                  # ended by eot inside decode()'s default sample_len
    assert margin > 100 * err32 > 0 and avg < 0 and 0 <= nsp <= 1
    c = R.Consts(k["n_vocab"], k["eot"], k["no_speech"], k["no_timestamps"], k["timestamp_begin"], k["max_initial_timestamp_index"], k["blank"],
                 k["suppress"])
    assert R.grammar_ok(c, greedy) and not set(greedy) & (set(k["suppress"]) | {eot})
    assert tok.decode(list(range(eot))) != ""      # every text id has a text: decode() can name any pick
    assert tok.encode(tok.decode(greedy)) != [] and len(tok.encode(" the")) == 1
    assert z["prompt9"].tolist() == synth.token_ids("whisper.dec.prompt.s", 9, eot, seed).tolist()


@pytest.mark.parametrize("rows", R.STEP_ROW_COUNTS)
def test_step_dispatch_families_at_small_en_width(rows):
    """What tests/test_gpu_whisper_widths.py asserts on the device, at 256 CUs and the default switches: a chooser change that would
    leave that test without the kernels it is there for fails here first."""
    cfg = synth.WHISPER_DEC_S
    names = R.step_dispatch(rows, cfg["d_model"], cfg["decoder_ffn_dim"], cfg["vocab_size"], cus=256, select_kernel=0, ring_mode=0, rows_ln_mode=2)
    R.check_small_en_step_families(rows, names)


def test_step_dispatch_covers_the_ln_and_lm_head_instantiations():
    """Over the row counts of the GPU test the LM head reaches five of the nine m16ln_stream instantiations below 33 rows and rows<mt>,
    tile64 above; the checkpoint widths reach m16ln<2> and m16ln<4> and are refused at 384 and 1280 (the two-call path)."""
    cfg = synth.WHISPER_DEC_S
    kw = dict(cus=256, select_kernel=0, ring_mode=0, rows_ln_mode=2)
    heads = {r: R.step_dispatch(r, 768, 3072, cfg["vocab_size"], **kw)["head"][1] for r in R.STEP_ROW_COUNTS}
    assert len({n for r, n in heads.items() if r <= 32}) == 5 and all(n.startswith("m16ln_stream<") for r, n in heads.items() if r <= 32)
    assert {n for r, n in heads.items() if r > 32} == {"rows<mt=1>", "rows<mt=2>", "tile64"}
    for width, want in ((384, None), (512, "m16ln<2,1,2>"), (1024, "m16ln<4,1,2>"), (1280, None)):
        for rows in (3, 40):
            names = R.step_dispatch(rows, width, 4 * width, 200, **kw)
            assert all(names[c + "_fused"] == (want is not None) and names[c][0] == 0 for c in ("qkv", "cross_q", "fc1", "head")), (width, rows, names)
            assert want is None or all(names[c][1] == want for c in ("qkv", "cross_q", "fc1", "head")), (width, rows, names)
            buf = ctypes.create_string_buffer(64)
            q = _lib.GemmF32Query.make("ln", rows, 3 * width, width, **kw)
            assert (_lib.load().hirest_gemm_f32_dispatch_name(ctypes.byref(q), buf, 64) == 0) == (want is not None), (width, rows)


def test_tokenizer_from_dir_and_load_model_from_pt(tmp_path):
    import json
    vocab, merges = synth.whisper_vocab(100)
    sp = synth.whisper_special_tokens(100)
    d = tmp_path / "tok"
    d.mkdir()
    (d / "vocab.json").write_text(json.dumps({**vocab, "<|endoftext|>": 100}), encoding="utf-8")
    (d / "merges.txt").write_text("#version: 0.2\n" + "\n".join(merges) + "\n", encoding="utf-8")
    added = {k: v for k, v in sp.items() if k != "<|endoftext|>"}
    added.update({f"<|{i * 0.02:.2f}|>": sp["<|notimestamps|>"] + 1 + i for i in range(88)})        # a Hugging Face file lists the timestamps too
    (d / "added_tokens.json").write_text(json.dumps(added), encoding="utf-8")
    tok = whisper.Tokenizer.from_dir(str(d))
    ref = synth.whisper_tokenizer(100)
    assert (tok.eot, tok.sot, tok.sot_prev, tok.no_speech, tok.timestamp_begin) == (ref.eot, ref.sot, ref.sot_prev, ref.no_speech, ref.timestamp_begin)
    assert tok.encode(" the (x)") == ref.encode(" the (x)") and tok.non_speech_tokens == ref.non_speech_tokens
    assert tok.decode_with_timestamps([tok.timestamp_begin + 3, 5]) == "<|0.06|>" + ref.decode([5])
    # an OpenAI checkpoint: dims + model_state_dict under OpenAI's names
    cfg, eot, seed, _ = synth.WHISPER_DEC_CASES["p"]
    hf = whisper.Whisper(cfg, {**{"encoder." + k: v for k, v in synth.whisper_encoder_state_dict(cfg, 3).items()},
                               **synth.whisper_decoder_state_dict(cfg, seed)})
    state = {**{"encoder." + k.replace("/", "."): v.data for k, v in hf.encoder._parameters.items()},
             **{"decoder." + k.replace("/", "."): v.data for k, v in hf.decoder._parameters.items()}}
    dims = {**hf.dims}
    path = tmp_path / "tiny.pt"
    torch.save({"dims": dims, "model_state_dict": state}, path)
    model = whisper.load_model(str(path), tokenizer=str(d))
    assert model.dims == hf.dims and model.tokenizer.eot == 100 and model.tokenizer.sot_sequence == (101,)
    assert all(torch.equal(v, model.decoder._parameters[k]) for k, v in hf.decoder._parameters.items())
    assert all(torch.equal(v, model.encoder._parameters[k]) for k, v in hf.encoder._parameters.items())


def test_initial_tokens(tok):
    f = whisper._initial_tokens
    assert f(tok, whisper.DecodingOptions(), 448) == ([tok.sot], 0)
    assert f(tok, whisper.DecodingOptions(prompt=[]), 448) == ([tok.sot], 0)                     # a file's first window: no sot_prev
    assert f(tok, whisper.DecodingOptions(without_timestamps=True), 448) == ([tok.sot, tok.no_timestamps], 0)
    long = list(range(300))
    got, sot_index = f(tok, whisper.DecodingOptions(prompt=long), 448)
    assert got == [tok.sot_prev] + long[-223:] + [tok.sot] and sot_index == 224                  # at most n_text_ctx / 2 - 1 previous tokens
    got, sot_index = f(tok, whisper.DecodingOptions(prompt=" the"), 448)
    assert got == [tok.sot_prev] + tok.encode(" the") + [tok.sot] and sot_index == 2
