"""Whisper's language handling on the device: ``hirest_whisper_language_tail`` against an fp64 restatement,
``detect_language`` against transformers' WhisperDecoder in fp64 (tests/golden/whisper_lang.npz), language and task in the prompt against
the lock-step loop (tests/_whisper_lockstep.py), detection inside ``decode`` / ``decode_many``, and ``transcribe(language=None)``.

Bars are yardsticks of the inputs themselves, as in tests/test_gpu_whisper_dec.py: 4 x the error of the same formula evaluated in fp32 on
the CPU against fp64, taken over the rows a case tests (the cases of 1 and 3 rows are the first rows of a pool of 17, so that a row
can be held bit-equal to itself in a larger call).  A row sum is held to that same bar.  The fp32 formula itself misses it — every
quotient carries the denominator's rounding error whole, up to 3.4e-7 at L = 99 against a bar of 8.5e-8 — which is why the kernel
takes the denominator and the quotients in double and rounds each probability once.  Everything else is equality.

Measured on an MI355X (printed by the tests; the bars are the yardsticks above, not these numbers): see DESIGN.md 4.18.
"""
import os
import wave

import numpy as np
import pytest
import torch

import _whisper_lang as L
from _whisper_lockstep import lockstep_decode
from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 1234.5
V, LD = 251, 256                   # the kernel tests' vocabulary and row stride: pad columns behind every row


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def table(n):
    return [7 + 2 * j for j in range(n)]                              # ascending, does not start at 0, every other column unused


def run_tail(logits, ids, dev, n_vocab=V):
    """one hirest_whisper_language_tail call on host logits [R, LD] -> (tokens [R], probs [R, L]) on the host; the outputs sit in
    canary-filled buffers with a row to spare"""
    lib = _lib.load()
    R_, n = logits.shape[0], len(ids)
    x, t = logits.to(dev).contiguous(), torch.tensor(ids, dtype=torch.int32, device=dev)
    tokens = torch.full((R_ + 1,), -7, dtype=torch.int32, device=dev)
    probs = torch.full((R_ + 1, n), CANARY, dtype=torch.float32, device=dev)
    _lib.check(lib.hirest_whisper_language_tail(x.data_ptr(), logits.shape[1], R_, n_vocab, t.data_ptr(), n, tokens.data_ptr(), probs.data_ptr(),
                                                ops.stream_ptr()), "hirest_whisper_language_tail")
    torch.cuda.synchronize()
    assert int(tokens[R_]) == -7 and bool((probs[R_] == CANARY).all()), "written past the rows"
    return tokens[:R_].cpu(), probs[:R_].cpu()


_POOLS = {}


def pool(n, dev):
    """per table size: 17 rows of seeded logits in [-3, 3), the fp64 restatement, the same in fp32 on the CPU, and the kernel's answer"""
    if n not in _POOLS:
        x = torch.from_numpy((synth.uniform_pm1("lang.logits", 17 * LD, 31 + n) * 3.0).astype(np.float32).reshape(17, LD))
        ids = table(n)
        p64, p32 = L.masked_softmax(x.numpy(), ids, np.float64), L.masked_softmax(x.numpy(), ids, np.float32).astype(np.float64)
        _POOLS[n] = (x, ids, p64, p32, run_tail(x, ids, dev))
    return _POOLS[n]


@pytest.mark.parametrize("R_", [1, 3, 17])
@pytest.mark.parametrize("n", [1, 4, 99, 100])
def test_language_tail_against_restatement(n, R_, dev):
    x, ids, p64, p32, (pool_tokens, pool_probs) = pool(n, dev)
    tokens, probs = run_tail(x[:R_], ids, dev)
    got = probs.double().numpy()
    yard = float(np.abs(p32[:R_] - p64[:R_]).max())                   # of the rows under test
    err, sum_err = float(np.abs(got - p64[:R_]).max()), float(np.abs(got.sum(-1) - 1.0).max())
    print(f"language tail L {n} R {R_}: max |prob - fp64| {err:.3e}, max |row sum - 1| {sum_err:.3e}, bar {4 * yard:.3e} (4 x fp32 CPU formula "
          f"{yard:.3e}); the fp32 formula's own row sums miss 1 by {float(np.abs(p32[:R_].sum(-1) - 1.0).max()):.3e}")
    assert not np.isnan(got).any()
    assert err <= 4 * yard
    assert sum_err <= 4 * yard
    cols = x[:R_].numpy().astype(np.float64)[:, ids]
    top = np.sort(cols, -1)
    margin = top[:, -1] - (top[:, -2] if n > 1 else -np.inf)
    clear = margin >= 100 * yard
    assert clear.all()                                                # seeded logits in [-3, 3): no row of the pool is a near-tie
    assert tokens.numpy()[clear].tolist() == [ids[j] for j in cols.argmax(-1)[clear]]
    # a row's bits do not depend on the rows beside it
    assert torch.equal(tokens, pool_tokens[:R_]) and torch.equal(probs, pool_probs[:R_])


@pytest.mark.parametrize("n", [4, 99, 100])
def test_language_tail_ties_go_to_the_lower_id(n, dev):
    x, ids, *_ = pool(n, dev)
    pairs = [(0, n - 1), (1, 2), (n - 2, n - 1)]
    if n > 64:
        pairs += [(5, 69), (70, 3), (63, 64)]                         # the two entries of one lane; across the halves of the table
    rows = x[:len(pairs)].clone()
    for r, (a, b) in enumerate(pairs):
        rows[r, ids[a]] = rows[r, ids[b]] = 5.0                       # two exact maxima
    tokens, probs = run_tail(rows, ids, dev)
    assert tokens.tolist() == [ids[min(a, b)] for a, b in pairs]
    for r, (a, b) in enumerate(pairs):
        assert probs[r, a] == probs[r, b] == probs[r].max()
    rows[:] = 0.25                                                    # every entry ties: the first id, and a uniform answer
    tokens, probs = run_tail(rows, ids, dev)
    assert tokens.tolist() == [ids[0]] * len(pairs) and bool((probs == probs[0, 0]).all()) and abs(float(probs[0, 0]) * n - 1.0) < 1e-6


@pytest.mark.parametrize("n", [1, 4, 99, 100])
def test_language_tail_saturates_to_one_and_zero(n, dev):
    ids = table(n)
    hot = [0, n - 1, n // 2]
    rows = torch.full((3, LD), -80.0)
    for r, j in enumerate(hot):
        rows[r, ids[j]] = 80.0
    tokens, probs = run_tail(rows, ids, dev)
    want = torch.zeros((3, n))
    for r, j in enumerate(hot):
        want[r, j] = 1.0
    assert not bool(torch.isnan(probs).any()) and torch.equal(probs, want) and tokens.tolist() == [ids[j] for j in hot]


@pytest.mark.parametrize("n", [1, 4, 100])
def test_language_tail_reads_only_the_table(n, dev):
    x, ids, _, _, (pool_tokens, pool_probs) = pool(n, dev)
    poisoned = torch.full_like(x, float("nan"))
    poisoned[:, ids] = x[:, ids]                                      # NaN in every other column, the pad columns included
    tokens, probs = run_tail(poisoned, ids, dev)
    assert torch.equal(tokens, pool_tokens) and torch.equal(probs, pool_probs)


# ---------------------------------------------------------------------------------------------------------------- detect_language
_STATE = {}


def fixture(dev):
    """(the multilingual case-q model, the fixture's windows on the device, the fixture)"""
    if not _STATE:
        _STATE["q"] = (L.model_for("q", dev), L.audio_states("q").to(dev), np.load(os.path.join(GOLDEN, "whisper_lang.npz")))
    return _STATE["q"]


def code_of(tok, token):
    return tok.all_language_codes[tok.all_language_tokens.index(int(token))]


def test_detect_language_equals_fixture(dev):
    model, xa, z = fixture(dev)
    tok = model.tokenizer
    tokens, probs = whisper.detect_language(model, xa)
    assert tokens.shape == (xa.shape[0],) and tokens.dtype == torch.int64 and [list(p) for p in probs] == [list(L.LANGS)] * len(probs)
    got = np.array([[p[c] for c in L.LANGS] for p in probs], dtype=np.float64)
    err, bar = float(np.abs(got - z["probs64"]).max()), 4 * float(z["probs_err32"])
    print(f"detect_language: winners {[code_of(tok, t) for t in tokens]}, max |prob - fp64| {err:.3e}, bar (4 x fp32 CPU forward) {bar:.3e}, "
          f"smallest margin of the fixture {float(z['margins'].min()):.3e}")
    assert tokens.tolist() == z["winners"].tolist()
    assert len(set(tokens.tolist())) >= 2                             # not a constant answer
    assert err <= bar
    assert model.detect_language(xa[:2])[0].tolist() == tokens[:2].tolist()
    with pytest.raises(ValueError, match="language tokens"):
        whisper.detect_language(model, xa[:1], synth.whisper_tokenizer(100))


@pytest.mark.parametrize("W", [2, 5])
def test_detect_language_rows_do_not_depend_on_their_neighbours(W, dev):
    model, xa, _ = fixture(dev)
    tokens, probs = whisper.detect_language(model, xa[:W])
    for w in range(W):
        t1, p1 = whisper.detect_language(model, xa[w])                # a single window: unbatched
        assert t1.ndim == 0 and isinstance(p1, dict)
        assert torch.equal(t1, tokens[w]) and p1 == probs[w], w
    perm = list(range(W))[::-1] if W == 2 else [3, 0, 4, 2, 1]
    tp, pp = whisper.detect_language(model, xa[perm])
    assert torch.equal(tp, tokens[perm]) and pp == [probs[i] for i in perm]
    assert whisper.detect_language(model, xa[:W])[1] == probs          # and on a second run


def test_detect_language_from_spectrograms(dev):
    model, _, _ = fixture(dev)
    cfg = synth.WHISPER_DEC_CASES["q"][0]
    mel = synth.whisper_mel_input(cfg, 3, 9).to(dev)                  # [3, 80, 522]: the synthetic encoder has 261 positions
    tokens, probs = whisper.detect_language(model, mel)
    ts, ps = whisper.detect_language(model, model.encoder(mel))
    assert torch.equal(tokens, ts) and probs == ps
    t1, p1 = whisper.detect_language(model, mel[1])
    assert torch.equal(t1, tokens[1]) and p1 == probs[1]


# ---------------------------------------------------------------------------------------------------------------- the prompt
def fields(r):
    return (r.tokens, r.text, r.avg_logprob, r.no_speech_prob, r.temperature, r.compression_ratio, r.language, r.language_probs)


def test_language_and_task_reach_the_prompt(dev, monkeypatch):
    model, xa, z = fixture(dev)
    tok = model.tokenizer
    opts = whisper.DecodingOptions(language="de", task="translate")
    res, cands = whisper.decode(model, xa[0], opts, return_candidates=True)
    plain, plain_cands = whisper.decode(model, xa[0], whisper.DecodingOptions(), return_candidates=True)
    initial, sot_index = whisper._initial_tokens(tok, opts, model.decoder.ctx)
    assert initial == [tok.sot, tok.to_language_token("de"), tok.translate] and sot_index == 0
    assert initial != whisper._initial_tokens(tok, whisper.DecodingOptions(), model.decoder.ctx)[0]
    # the yardstick: the lock-step loop, whose prompt is its tokenizer's own
    monkeypatch.setattr(model, "tokenizer", tok.with_language("de", "translate"))
    want_cands, want_nsp = lockstep_decode(model, xa[0], whisper.DecodingOptions())
    monkeypatch.undo()
    assert cands == want_cands and res.no_speech_prob == want_nsp and res.tokens == want_cands[0][0]
    assert res.language == "de" and plain.language == "en" and res.language_probs is None
    print(f"de / translate: {len(res.tokens)} tokens, sum_logprobs {cands[0][1]:.6f}; en / transcribe: {len(plain.tokens)} tokens, "
          f"sum_logprobs {plain_cands[0][1]:.6f}")
    assert cands != plain_cands                                       # the prompt matters
    # no_speech_prob is read at <|startoftranscript|>, which precedes both prompts' language: the same bits, and the fixture's value
    assert res.no_speech_prob == plain.no_speech_prob
    print(f"no_speech_prob {res.no_speech_prob:.9f} (fp64 {float(z['no_speech64'][0]):.9f}, bar {4 * float(z['no_speech_err32']):.3e})")
    assert abs(res.no_speech_prob - float(z["no_speech64"][0])) <= 4 * float(z["no_speech_err32"])


def test_decode_detects_an_undetermined_language(dev, monkeypatch):
    model, xa, z = fixture(dev)
    tok = model.tokenizer
    winners = [code_of(tok, t) for t in z["winners"]]
    a, b = 0, next(w for w in range(len(winners)) if winners[w] != winners[0])          # two windows of different languages
    given = {w: whisper.decode(model, xa[w], whisper.DecodingOptions(language=winners[w]), return_candidates=True) for w in (a, b)}
    detected = {w: whisper.detect_language(model, xa[w])[1] for w in (a, b)}
    monkeypatch.setattr(model, "tokenizer", tok.with_language(None, "transcribe"))
    for w in (a, b):
        res, cands = whisper.decode(model, xa[w], return_candidates=True)
        assert res.language == winners[w] and res.language_probs == detected[w]
        assert cands == given[w][1] and fields(res)[:6] == fields(given[w][0])[:6]
        assert given[w][0].language == winners[w] and given[w][0].language_probs is None
    many = whisper.decode_many(model, xa[[a, b]])
    assert [r.language for r in many] == [winners[a], winners[b]] and winners[a] != winners[b]
    for r, w in zip(many, (a, b)):
        assert fields(r) == fields(whisper.decode(model, xa[w])), w
    # the same with the languages given per window in one call
    per_window = whisper.decode_many(model, xa[[a, b]], [whisper.DecodingOptions(language=winners[a]), whisper.DecodingOptions(language=winners[b])])
    for r, w in zip(per_window, (a, b)):
        assert fields(r) == fields(given[w][0]), w
    # and one window of each kind in a call: only the undetermined one is detected
    mixed = whisper.decode_many(model, xa[[a, b]], [whisper.DecodingOptions(), whisper.DecodingOptions(language=winners[b])])
    assert fields(mixed[0]) == fields(many[0]) and fields(mixed[1]) == fields(given[b][0])


# ---------------------------------------------------------------------------------------------------------------- transcribe
def write_wav(path, audio):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(audio, -1, 1 - 1 / 32768) * 32768).astype("<i2").tobytes())
    return str(path)


def test_transcribe_detects_the_language_of_a_file(dev, tmp_path):
    """case p's decoder behind the 1500-position synthetic encoder, as test_transcribe_end_to_end builds it, with the multilingual
    tokenizer in the state load_model leaves it (language "en"): language=None detects on the first window"""
    model = L.model_for("p", dev, synth.WHISPER_E2E)
    tok = model.tokenizer
    paths = [write_wav(tmp_path / "a.wav", synth.audio_clip("mixed", 31 * 16000, 71)),
             write_wav(tmp_path / "b.wav", synth.audio_clip("noise", 12 * 16000, 72))]
    kw = dict(temperature=(0.0, 0.4), best_of=5, compression_ratio_threshold=2.4, logprob_threshold=-1.0, no_speech_threshold=0.6)
    outs = []
    for path in paths:
        mel = whisper.log_mel_spectrogram(path, 80, padding=whisper.N_SAMPLES, device=dev)
        token, probs = whisper.detect_language(model, whisper.pad_or_trim(mel[:, :whisper.N_FRAMES], whisper.N_FRAMES))
        out = whisper.transcribe(model, path, language=None, **kw)
        print(f"transcribe {os.path.basename(path)}: language {out['language']} ({probs}), {len(out['segments'])} segments")
        assert out["language"] == code_of(tok, token)
        assert out == whisper.transcribe(model, path, language=out["language"], **kw)
        outs.append(out)
    assert whisper.transcribe_many(model, paths, language=None, files_in_flight=2, **kw) == outs
