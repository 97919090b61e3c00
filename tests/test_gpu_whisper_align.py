"""Word-level timestamps on the device: hirest_whisper_alignment_matrix against the fp64 restatement with the fp32 CPU
evaluation of the same formulas as the yardstick, its median step against numpy's median exactly, hirest_dtw_f32 against the numpy
recurrence in fp32 exactly (path and cost), find_alignment on the synthetic decoder cases, and transcribe(word_timestamps=True)."""
import copy
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

import _whisper_align_ref as A
import test_gpu_whisper_dec as S
from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- the matrix
_INPUTS = {}


def inputs(H, T, Tk, seed):
    """two layers of cross-attention query rows [T, D] and key | value rows [Tk, 2 D], seeded like synth.whisper_audio_states (unit
    scale): built once per shape, never modified"""
    key = (H, T, Tk, seed)
    if key not in _INPUTS:
        D = 64 * H
        _INPUTS[key] = ([synth.tensor(f"align.q.{l}", (T, D), 1.0, seed) for l in range(2)],
                        [synth.tensor(f"align.kv.{l}", (Tk, 2 * D), 1.0, seed + 1) for l in range(2)])
    return _INPUTS[key]


def pairs_for(H, which):
    if which == "one":
        return [(1, H - 1)]
    if which == "three":                                              # crossing two layers, not in layer order
        return [(1, 0), (0, H - 1), (1, 1)]
    return [(l, h) for l in range(2) for h in range(H)]


# (H, pairs, T, n_keys, Tk, medfilt_width, row0, n_rows, qk_scale, seed).  T = 2 goes with few columns: a column of two tokens has a
# spread worth dividing by only when the two differ, which a seed can arrange for tens of columns and not for thousands.
MATRIX_CASES = [
    (2, "three", 2, 7, 9, 7, 1, 1, 1.0, 11),
    (2, "three", 9, 3, 8, 7, 2, 7, 1.0, 12),         # 3 <= 7 // 2: unfiltered
    (2, "three", 9, 4, 8, 7, 2, 7, 0.5, 12),         # the shortest filtered row: the reflection reaches the other end
    (2, "all", 9, 7, 7, 7, 1, 8, 0.5, 13),
    (12, "all", 70, 33, 33, 7, 1, 69, 1.0, 14),
    (12, "three", 9, 64, 70, 1, 3, 5, 1.0, 15),      # one full chunk, width 1
    (12, "one", 70, 65, 70, 7, 2, 68, 0.5, 16),      # a chunk and one key
    (2, "all", 70, 261, 300, 7, 3, 60, 1.0, 17),     # a second median tile of five keys
    (12, "all", 9, 1500, 1500, 7, 1, 8, 1.0, 18),
    (2, "three", 9, 1500, 1501, 1, 4, 5, 0.5, 19),
]


def run_matrix(q, kv, pairs, n_keys, H, dev, workspace=None, **kw):
    """the kernel on device copies whose keys past n_keys (and every value column) are NaN: nothing may depend on them"""
    D = 64 * H
    kv_dev = []
    for t in kv:
        c = t.clone()
        c[n_keys:] = float("nan")
        c[:, D:] = float("nan")
        kv_dev.append(c.to(dev))
    return whisper.alignment_matrix([t.to(dev) for t in q], kv_dev, pairs, n_keys, heads=H, workspace=workspace, **kw)


@pytest.mark.parametrize("case", MATRIX_CASES, ids=lambda c: "H{}-{}-T{}-n{}of{}-w{}-r{}+{}-s{}".format(*c[:9]))
def test_alignment_matrix_against_fp64(case, dev):
    H, which, T, n_keys, Tk, width, row0, n_rows, qk_scale, seed = case
    q, kv = inputs(H, T, Tk, seed)
    pairs = pairs_for(H, which)
    args = dict(qk_scale=qk_scale, medfilt_width=width, row0=row0, n_rows=n_rows)
    qn, kvn = [t.numpy() for t in q], [t.numpy() for t in kv]
    want = A.alignment_matrix(qn, kvn, pairs, n_keys, dtype=np.float64, **args)       # (asserts every column's spread itself)
    cpu32 = A.alignment_matrix(qn, kvn, pairs, n_keys, dtype=np.float32, **args)
    got = run_matrix(q, kv, pairs, n_keys, H, dev, **args)
    assert got.shape == want.shape == (n_rows, n_keys) and bool(torch.isfinite(got).all())
    err, err32 = float(np.abs(got.cpu().double().numpy() - want).max()), float(np.abs(cpu32.astype(np.float64) - want).max())
    print(f"alignment matrix {case}: max |got - fp64| {err:.3e}, the same formulas in fp32 on the CPU {err32:.3e}, bar {4 * err32:.3e}, "
          f"|matrix| max {float(np.abs(want).max()):.2f}")
    assert err <= 4 * err32
    again = run_matrix(q, kv, pairs, n_keys, H, dev, **args)
    assert torch.equal(got, again)


def test_alignment_matrix_of_one_key_is_undefined_as_defined(dev):
    """n_keys = 1: a softmax over one key is exactly 1 for every token, the column's standard deviation exactly 0, and 0 / 0 is what
    the definition (and Whisper) gives.  The case is here for its bounds — one key of a window of five, the rest NaN — and because the
    restatement's spread assertion can hold for no seed."""
    q, kv = inputs(2, 2, 5, 10)
    got = run_matrix(q, kv, pairs_for(2, "one"), 1, 2, dev, medfilt_width=7, row0=1, n_rows=1)
    assert got.shape == (1, 1) and bool(torch.isnan(got).all())
    with np.errstate(invalid="ignore"), pytest.raises(AssertionError, match="standard deviation"):
        A.alignment_matrix([t.numpy() for t in q], [t.numpy() for t in kv], pairs_for(2, "one"), 1, medfilt_width=7, row0=1, n_rows=1)


def test_alignment_matrix_does_not_depend_on_the_workspace_before(dev):
    H, T = 2, 9
    q1, kv1 = inputs(H, T, 300, 21)
    q2, kv2 = inputs(H, 70, 300, 22)
    pairs = pairs_for(H, "all")
    lib = _lib.load()
    ws = torch.empty((int(lib.hirest_whisper_alignment_workspace_bytes(len(pairs), 70, 300)),), dtype=torch.uint8, device=dev)
    alone = run_matrix(q1, kv1, pairs, 261, H, dev, row0=1, n_rows=8)
    ws.fill_(0xFF)                                                    # NaN bit patterns in every float of it
    first = run_matrix(q1, kv1, pairs, 261, H, dev, workspace=ws, row0=1, n_rows=8)
    other = run_matrix(q2, kv2, pairs, 300, H, dev, workspace=ws, row0=0, n_rows=70)
    after = run_matrix(q1, kv1, pairs, 261, H, dev, workspace=ws, row0=1, n_rows=8)
    assert torch.equal(alone, first) and torch.equal(alone, after) and bool(torch.isfinite(other).all())
    small = torch.empty((16,), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="WORKSPACE"):
        run_matrix(q1, kv1, pairs, 261, H, dev, workspace=small)
    with pytest.raises(RuntimeError, match="BADARG"):
        run_matrix(q1, kv1, pairs, 301, H, dev)                       # more keys than the window has
    with pytest.raises(RuntimeError, match="BADARG"):
        run_matrix(q1, kv1, pairs, 261, H, dev, medfilt_width=4)


@pytest.mark.parametrize("width", [1, 3, 7, 31])
def test_median_step_equals_numpy_median(width, dev):
    """the median and mean steps alone (hirest_median_filter_mean_f32 with one head: the mean of one value is the value): equal to
    numpy's median over the reflect-padded windows of the same fp32 data, ties included (values on a grid of 1/4)"""
    for n in (1, 3, 4, 15, 16, 17, 256, 257, 300):
        x = np.round(synth.uniform_pm1(f"align.median.{n}", 5 * n, 31).reshape(5, n) * 8.0).astype(np.float32) / 4.0
        x[0] = synth.uniform_pm1(f"align.median.real.{n}", n, 32).astype(np.float32)
        got = whisper.median_filter(torch.from_numpy(x).to(dev), width)
        pad = width // 2
        if n <= pad:
            want = x
        else:
            want = np.median(np.lib.stride_tricks.sliding_window_view(np.pad(x, [(0, 0), (pad, pad)], mode="reflect"), width, axis=-1), axis=-1)
        assert want.dtype == np.float32 and torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want))), (width, n)
        assert np.array_equal(A.median_filter(x, width), want)
    # three heads: the mean in ascending head order, one fp32 addition per head and one division
    w = synth.tensor("align.median.heads", (3, 4, 70), 1.0, 33)
    out = torch.empty((2, 70), dtype=torch.float32, device=dev)
    wd = w.to(dev)
    _lib.check(_lib.load().hirest_median_filter_mean_f32(wd.data_ptr(), 3, 4, 70, width, 1, 2, out.data_ptr(), ops.stream_ptr()), "median")
    f = A.median_filter(w.numpy(), width)[:, 1:3]
    want = ((f[0] + f[1]) + f[2]) / np.float32(3)
    assert torch.equal(out.cpu(), torch.from_numpy(want))


# ---------------------------------------------------------------------------------------------------------------- dtw
def dtw_input(N, M, kind, seed=41):
    u = synth.uniform_pm1(f"align.dtw.{N}.{M}.{kind}", N * M, seed).reshape(N, M)
    return (np.round(u * 2.0) if kind == "integer" else u * 3.0).astype(np.float32)


_DTW_REF = {}


def dtw_ref(N, M, kind, negate=False):
    key = (N, M, kind, negate)
    if key not in _DTW_REF:
        x = dtw_input(N, M, kind)
        _DTW_REF[key] = A.dtw(-x if negate else x, dtype=np.float32, return_cost=True)
    return _DTW_REF[key]


DTW_SIZES = [(1, 1), (1, 65), (2, 1), (2, 2), (63, 64), (64, 65), (65, 2), (65, 64), (64, 300), (256, 300), (225, 1500)]


@pytest.mark.parametrize("kind", ["real", "integer"])
@pytest.mark.parametrize("N,M", DTW_SIZES)
def test_dtw_equals_the_fp32_recurrence(N, M, kind, dev):
    x = dtw_input(N, M, kind)
    ti, tj, cost = dtw_ref(N, M, kind)
    (gi, gj, gcost), = whisper.dtw_many([torch.from_numpy(x).to(dev)], return_cost=True)
    assert gi.tolist() == ti.tolist() and gj.tolist() == tj.tolist()
    assert torch.equal(gcost.cpu(), torch.from_numpy(cost))           # every cell: the bits of the sequential evaluation
    assert (gi[0], gj[0], gi[-1], gj[-1]) == (0, 0, N - 1, M - 1) and len(gi) <= N + M - 1
    hi, hj = whisper.dtw(torch.from_numpy(x).to(dev))                 # without the cost output
    assert hi.tolist() == ti.tolist() and hj.tolist() == tj.tolist()


def test_dtw_negated_strided_and_batched(dev):
    sizes = [(65, 300, "real"), (9, 64, "integer"), (225, 70, "real")]          # the last: N > M
    wide = [torch.full((N + 2, M + 5), float("nan"), dtype=torch.float32) for N, M, _ in sizes]
    for w, (N, M, kind) in zip(wide, sizes):
        w[1:N + 1, 2:M + 2] = torch.from_numpy(dtw_input(N, M, kind))
    views = [w.to(dev)[1:N + 1, 2:M + 2] for w, (N, M, _) in zip(wide, sizes)]  # a row stride of M + 5, NaN around the matrix
    assert all(v.stride(0) == v.shape[1] + 5 for v in views)
    together = whisper.dtw_many(views, negate=True, return_cost=True)
    for (N, M, kind), v, (gi, gj, gcost) in zip(sizes, views, together):
        ti, tj, cost = dtw_ref(N, M, kind, negate=True)
        assert gi.tolist() == ti.tolist() and gj.tolist() == tj.tolist() and torch.equal(gcost.cpu(), torch.from_numpy(cost)), (N, M)
        (ai, aj, acost), = whisper.dtw_many([v], negate=True, return_cost=True)                 # alone: the same
        assert ai.tolist() == gi.tolist() and aj.tolist() == gj.tolist() and torch.equal(acost, gcost)
    plain = whisper.dtw((-views[1]).contiguous())
    assert plain[0].tolist() == together[1][0].tolist() and plain[1].tolist() == together[1][1].tolist()


def test_dtw_refuses_sizes_outside_the_limits(dev):
    lib = _lib.load()
    x = torch.zeros((8, 8), dtype=torch.float32, device=dev)
    path = torch.full((20, 2), -7, dtype=torch.int32, device=dev)
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device=dev)
    p = (_lib.DtwProblem * 1)()
    for N, M in ((0, 8), (257, 8), (8, 0), (8, 4097), (-1, 8)):
        p[0].x, p[0].ldx, p[0].N, p[0].M, p[0].path, p[0].path_len = x.data_ptr(), 8, N, M, path.data_ptr(), path[19].data_ptr()
        assert lib.hirest_dtw_f32(p, 1, ws.data_ptr(), ws.numel(), ops.stream_ptr()) == -1, (N, M)
    p[0].N, p[0].M = 8, 8
    assert lib.hirest_dtw_f32(p, 1, ws.data_ptr(), 16, ops.stream_ptr()) == -3                 # the workspace is too small
    p[0].ldx = 7
    assert lib.hirest_dtw_f32(p, 1, ws.data_ptr(), ws.numel(), ops.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((path == -7).all())                                   # nothing was launched
    with pytest.raises(ValueError):
        whisper.dtw(torch.zeros((257, 4), device=dev))


# ---------------------------------------------------------------------------------------------------------------- find_alignment
def model(case, dev):
    if case not in S._MODELS:
        S._MODELS[case] = S.model_for(case, dev)
    return S._MODELS[case]


@pytest.mark.parametrize("case", ["p", "q", "s"])
def test_find_alignment_on_the_synthetic_decoders(case, dev):
    m = model(case, dev)
    _, xa, _, _, _ = S.decoder(case, dev)
    z = np.load(os.path.join(GOLDEN, f"whisper_align_{case}.npz"))
    tok, Tk = m.tokenizer, int(xa.shape[1])
    greedy = whisper.decode(m, xa[0], whisper.DecodingOptions(temperature=0.0)).tokens
    assert [t for t in greedy if t < tok.eot] == z["greedy_text"].tolist()
    by_token = copy.copy(tok)                                         # every token a word: a jump of the path per token is read
    by_token.split_to_word_tokens = by_token.split_tokens_on_unicode
    runs = [("greedy", tok, 2 * Tk), ("greedy", by_token, 2 * Tk), ("extra", tok, 2 * Tk), ("extra", by_token, 2 * (Tk - 5) + 1)]
    for name, tokenizer, num_frames in runs:
        text = z[name + "_text"].tolist()
        details = {}
        got = whisper.find_alignment(m, tokenizer, text, xa[0], num_frames, details=details)
        if not text:                                                  # case p's greedy window has timestamps only
            assert got == [] and not details
            continue
        matrix = details["matrix"].cpu().numpy()
        assert matrix.shape == (len(text) + 1, num_frames // 2) and np.isfinite(matrix).all()
        # times: from the kernel's own fp32 matrix through the reference dtw and the reference word logic, exactly
        ti, tj = A.dtw(-matrix, dtype=np.float32)
        assert details["text_indices"].tolist() == ti.tolist() and details["time_indices"].tolist() == tj.tolist()
        words, word_tokens = tokenizer.split_to_word_tokens(text + [tok.eot])
        want = A.words_from_path(words, word_tokens, ti, tj, z[name + "_probs64"])
        assert len(got) == len(want) == len(words) - 1 >= 1
        bar = 4 * float(z[name + "_err32"])
        err = float(np.abs(details["token_probs"].astype(np.float64) - z[name + "_probs64"]).max())
        print(f"find_alignment {case} {name} ({len(got)} words, {num_frames // 2} keys): token probabilities max |got - fp64| {err:.3e}, bar {bar:.3e}; "
              f"times {[(w.start, w.end) for w in got][:6]}")
        assert err <= bar
        for g, (word, tokens, start, end, prob) in zip(got, want):
            assert (g.word, g.tokens, g.start, g.end) == (word, tokens, start, end)
            assert abs(g.probability - prob) <= bar
        assert all(a.end == b.start for a, b in zip(got, got[1:])) and got[0].start >= 0 and got[-1].end <= (num_frames // 2) / 50
    # another set of heads changes the matrix, and the call says so
    if m.decoder.heads > 1:
        d0, d1 = {}, {}
        text = z["extra_text"].tolist()
        whisper.find_alignment(m, by_token, text, xa[0], 2 * Tk, details=d0)
        keep = m.alignment_heads.clone()
        m.set_alignment_heads([(m.decoder.layers - 1, 0)])
        try:
            whisper.find_alignment(m, by_token, text, xa[0], 2 * Tk, details=d1)
        finally:
            m.set_alignment_heads(keep)
        assert not torch.equal(d0["matrix"], d1["matrix"])
    assert tuple(m.alignment_heads.shape) == (m.decoder.layers, m.decoder.heads)
    assert m.alignment_heads.nonzero().tolist() == [[l, h] for l in range(m.decoder.layers // 2, m.decoder.layers) for h in range(m.decoder.heads)]


# ---------------------------------------------------------------------------------------------------------------- transcribe
_E2E = {}


def e2e(dev, tmp_path_factory):
    """the model behind the 1500-position encoder and two inputs of about 12 s and 31 s (the second as a .wav file), transcribed without
    and with word timestamps: built once"""
    if not _E2E:
        m = S.model_for("p", dev, synth.WHISPER_E2E)
        clips = [synth.audio_clip("mixed", int(s * 16000), seed) for s, seed in ((12.3, 5), (31.0, 71))]
        path = str(tmp_path_factory.mktemp("align") / "clip.wav")
        with wave.open(path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(clips[1], -1, 1 - 1 / 32768) * 32768).astype("<i2").tobytes())
        audios = [clips[0], path]
        kw = dict(temperature=(0.0, 0.4), best_of=5)
        _E2E.update(model=m, audios=audios, kw=kw, off=[whisper.transcribe(m, a, **kw) for a in audios],
                    on=[whisper.transcribe(m, a, word_timestamps=True, **kw) for a in audios])
    return _E2E


def test_transcribe_with_word_timestamps(dev, tmp_path_factory):
    e = e2e(dev, tmp_path_factory)
    n_words = 0
    for on, off in zip(e["on"], e["off"]):
        assert on["text"] == off["text"] and on["language"] == off["language"] and len(on["segments"]) == len(off["segments"])
        for a, b in zip(on["segments"], off["segments"]):
            assert "words" in a and "words" not in b
            assert {k: v for k, v in a.items() if k != "words"} == b
            words = a["words"]
            assert "".join(w["word"] for w in words) == a["text"]
            times = [t for w in words for t in (w["start"], w["end"])]
            assert times == sorted(times) and all(a["start"] <= t <= a["end"] for t in times), (a["start"], a["end"], times)
            assert all(0.0 <= w["probability"] <= 1.0 for w in words)
            n_words += len(words)
    print(f"transcribe(word_timestamps=True): {[len(r['segments']) for r in e['on']]} segments, {n_words} words; first words "
          f"{[(w['word'], w['start'], w['end']) for r in e['on'] for s in r['segments'][:1] for w in s['words'][:4]]}")
    assert n_words > 0


def test_transcribe_many_gives_the_same_words(dev, tmp_path_factory):
    e = e2e(dev, tmp_path_factory)
    got = whisper.transcribe_many(e["model"], e["audios"], files_in_flight=2, word_timestamps=True, **e["kw"])
    assert len(got) == 2
    for g, w in zip(got, e["on"]):
        assert g["text"] == w["text"] and g["segments"] == w["segments"]
