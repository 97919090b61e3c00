"""The Whisper text decoder on the device (csrc/whisper_dec.hip, hirest_amd/whisper.py): the split-key cross-attention kernel, the
in-place self-attention form, the step tail, the decoder against transformers' WhisperDecoder in fp64 (tests/golden/whisper_dec_*.npz),
greedy and sampled decode() and transcribe() end to end.  Inputs and weights are rebuilt from hirest_amd.synth; nothing here needs
transformers.  Bars are yardsticks of the inputs themselves — the error of the same formula evaluated in fp32 on the CPU against fp64,
times 4 — never figures of the kernels.

Measured on an MI355X (printed by the tests; the bars are the yardsticks above, not these numbers):
    cross-attention  max |got - fp64| / yard (bar 4): Tk 33 1.28 / 1.20 (H 2 / 4), Tk 261 0.85 / 0.68, Tk 1500 0.66 / 0.71, Tk 1 exact
    tail             worst |logprob, sum, no_speech - fp64| 3.9e-7 (V 200, bar 1.1e-6) / 1.0e-6 (V 51864, bar 5.4e-6); 0 of 160 sampled
                     draws under the margin bar; chi-square 8.06 (15 degrees of freedom)
    decoder          max |got - fp64| / the fp32 CPU forward's error (bar 4): p 0.74, q 0.61, r 1.33

"""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

import _whisper_dec_ref as R
from hirest_amd import _lib, dataset, ops, synth, whisper

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 1234.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def seeded(name, shape, seed, scale=1.0):
    return torch.from_numpy((synth.uniform_pm1(name, int(np.prod(shape)), seed) * scale).astype(np.float32).reshape(shape))


# ---------------------------------------------------------------------------------------------------------------- cross-attention
def run_cross(q, kv, row_window, H, Tk, dev):
    """q [R, H * 64], kv [W, Tk, 2 * H * 64] (host) -> out [R, H * 64] (host); workspace and output sit in canary-filled buffers"""
    lib = _lib.load()
    R_, D = q.shape
    need = lib.hirest_attention_f32_cross_decode_workspace_bytes(R_, H, Tk)
    assert need == R_ * H * ((Tk + 63) // 64) * 68 * 4
    ws = torch.full((need // 4 + 64,), CANARY, dtype=torch.float32, device=dev)
    out = torch.full((R_ + 1, D + 4), CANARY, dtype=torch.float32, device=dev)          # a row stride wider than the row, and a row after
    qd, kvd, rw = q.to(dev), kv.to(dev), torch.tensor(row_window, dtype=torch.int32, device=dev)
    _lib.check(lib.hirest_attention_f32_cross_decode(qd.data_ptr(), D, kvd.data_ptr(), 2 * D, Tk * 2 * D, kv.shape[0], Tk, rw.data_ptr(),
                                                     out.data_ptr(), D + 4, R_, H, 0.125, ws.data_ptr(), need, ops.stream_ptr()),
               "hirest_attention_f32_cross_decode")
    torch.cuda.synchronize()
    assert bool((ws[need // 4:] == CANARY).all()), "the workspace was written past its declared size"
    assert bool((out[:R_, D:] == CANARY).all()) and bool((out[R_] == CANARY).all()), "the output was written outside its rows"
    return out[:R_, :D].cpu()


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("Tk", [1, 33, 261, 1500])
def test_cross_decode(Tk, H, dev):
    D = 64 * H
    kv = seeded("xdec.kv", (2, Tk, 2 * D), 7 * Tk + H, 1.5)
    q = seeded("xdec.q", (7, D), 11 * Tk + H, 4.0)
    windows7 = [0, 1, 0, 0, 1, 1, 0]                                  # 7 rows over 2 windows
    got7 = run_cross(q, kv, windows7, H, Tk, dev)
    k = kv[..., :D].reshape(2, Tk, H, 64).numpy()
    v = kv[..., D:].reshape(2, Tk, H, 64).numpy()
    err = yard = 0.0
    for r in range(7):
        w = windows7[r]
        ref = R.cross_attention(q[r].view(H, 64).numpy(), k[w], v[w], 0.125, np.float64)
        f32 = R.cross_attention(q[r].view(H, 64).numpy(), k[w], v[w], 0.125, np.float32)
        err = max(err, float(np.abs(got7[r].view(H, 64).numpy().astype(np.float64) - ref).max()))
        yard = max(yard, float(np.abs(f32.astype(np.float64) - ref).max()))
    print(f"cross-decode Tk {Tk} H {H}: max |got - fp64| {err:.3e}, fp32 CPU formula {yard:.3e}, ratio {err / yard if yard else 0.0:.2f}")
    assert err <= 4 * yard
    # a row's bits do not depend on what else is in the call: alone, among 5 rows of one window, permuted, and on a second run
    for r in range(7):
        alone = run_cross(q[r:r + 1], kv, [windows7[r]], H, Tk, dev)
        assert torch.equal(alone[0], got7[r]), r
    rows5 = [0, 2, 3, 6, 2]                                           # 5 rows of window 0 (one of them twice)
    got5 = run_cross(q[rows5], kv[:1], [0] * 5, H, Tk, dev)
    assert torch.equal(got5, got7[rows5])
    perm = [6, 4, 5, 0, 3, 1, 2]
    assert torch.equal(run_cross(q[perm], kv, [windows7[i] for i in perm], H, Tk, dev), got7[perm])
    assert torch.equal(run_cross(q, kv, windows7, H, Tk, dev), got7)
    # a row that names no window gets zeros and disturbs nobody
    odd = run_cross(q[:3], kv, [0, 5, 0], H, Tk, dev)
    assert torch.equal(odd[0], got7[0]) and torch.equal(odd[2], got7[2]) and bool((odd[1] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- in-place self-attention
@pytest.mark.parametrize("t", [0, 1, 63, 64, 65, 223])
def test_decode_inplace_equals_decode(t, dev):
    lib = _lib.load()
    R_, H, T_max = 3, 2, 224
    D = 64 * H
    hist_k, hist_v = seeded("inpl.k", (R_, T_max, D), 3, 1.5).to(dev), seeded("inpl.v", (R_, T_max, D), 4, 1.0).to(dev)
    qkv = seeded("inpl.qkv", (R_, 3 * D), 5 + t, 3.0).to(dev)
    want = torch.empty((R_, D), dtype=torch.float32, device=dev)
    pk, pv = hist_k[:, :t].contiguous(), hist_v[:, :t].contiguous()
    _lib.check(lib.hirest_attention_f32_decode(qkv.data_ptr(), 3 * D, pk.data_ptr() if t else None, pv.data_ptr() if t else None, D, None, t,
                                               qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, None, None, want.data_ptr(), R_, H, 0.125,
                                               0.0, 0.0, ops.stream_ptr()), "hirest_attention_f32_decode")
    ck = torch.full((R_, T_max, D), CANARY, dtype=torch.float32, device=dev)
    cv = torch.full((R_, T_max, D), CANARY, dtype=torch.float32, device=dev)
    ck[:, :t], cv[:, :t] = hist_k[:, :t], hist_v[:, :t]
    before_k, before_v = ck.clone(), cv.clone()
    got = torch.empty((R_, D), dtype=torch.float32, device=dev)
    _lib.check(lib.hirest_attention_f32_decode_inplace(qkv.data_ptr(), 3 * D, ck.data_ptr(), cv.data_ptr(), D, T_max * D, t, T_max,
                                                       qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, got.data_ptr(), R_, H, 0.125, 0.0, 0.0,
                                                       ops.stream_ptr()), "hirest_attention_f32_decode_inplace")
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(ck[:, t], qkv[:, D:2 * D]) and torch.equal(cv[:, t], qkv[:, 2 * D:])          # the appended row
    before_k[:, t], before_v[:, t] = ck[:, t], cv[:, t]
    assert torch.equal(ck, before_k) and torch.equal(cv, before_v)                                   # and nothing else
    assert lib.hirest_attention_f32_decode_inplace(qkv.data_ptr(), 3 * D, ck.data_ptr(), cv.data_ptr(), D, T_max * D, T_max, T_max,
                                                   qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, got.data_ptr(), R_, H, 0.125, 0.0, 0.0,
                                                   ops.stream_ptr()) == -2                           # a full cache is refused, not overrun


# ---------------------------------------------------------------------------------------------------------------- the tail
def consts_for(V):
    eot = 100 if V == 200 else 50256
    sp = synth.whisper_special_tokens(eot)
    nts = sp["<|notimestamps|>"]
    sup = [5, 17, 60, sp["<|startoftranscript|>"], sp["<|startofprev|>"], sp["<|startoflm|>"], sp["<|transcribe|>"], sp["<|translate|>"],
           sp["<|nospeech|>"]]
    return R.Consts(V, eot, sp["<|nospeech|>"], nts, nts + 1, 9, blank=3, suppress=sup)


def tail_call(c, logits, seqs, completed, sum0, dev, temperature=0.0, seed=0, serial=0, step=0, want_logprobs=True, n_vocab=None):
    """one hirest_whisper_step_tail call on host logits [R, V] and per-row histories; returns host copies of everything it wrote"""
    lib = _lib.load()
    R_, V = logits.shape
    words = np.zeros((V + 31) // 32, dtype=np.uint32)
    for t in list(c.suppress) + list(range(n_vocab or V, V)):
        words[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    mask = torch.from_numpy(words.view(np.int32)).to(dev)
    p = _lib.WhisperTailParams()
    p.n_vocab, p.eot, p.no_speech, p.no_timestamps, p.timestamp_begin = n_vocab or V, c.eot, c.no_speech, c.no_timestamps, c.timestamp_begin
    p.max_initial_timestamp_index = -1 if c.max_initial_timestamp_index is None else c.max_initial_timestamp_index
    p.sample_begin, p.blank, p.suppress_blank, p.timestamp_rules, p.monotonic = 2, c.blank, int(c.suppress_blank), int(c.timestamp_rules), int(c.monotonic)
    p.temperature, p.seed, p.serial, p.suppress_mask = temperature, seed, serial, mask.data_ptr()
    st = torch.zeros((R_, 8), dtype=torch.int32)
    for r, seq in enumerate(seqs):
        stamps = [t for t in seq if t >= c.timestamp_begin]
        st[r, :5] = torch.tensor([len(seq), seq[-1] if seq else -1, seq[-2] if len(seq) > 1 else -1, stamps[-1] if stamps else -1, int(completed[r])])
    st[:, 5] = torch.tensor(sum0, dtype=torch.float32).view(torch.int32)
    st = st.to(dev)
    T_max = 8
    x = logits.to(dev)
    ids = torch.full((R_ + 1,), -7, dtype=torch.int32, device=dev)
    toks = torch.full((R_ + 1, T_max), -7, dtype=torch.int32, device=dev)
    lps = torch.full((R_ + 1, V), CANARY, dtype=torch.float32, device=dev) if want_logprobs else None
    stamp = torch.zeros(1, dtype=torch.int32).pin_memory()
    _lib.check(lib.hirest_whisper_step_tail(x.data_ptr(), V, R_, V, step, T_max, C.byref(p), st.data_ptr(), ids.data_ptr(), toks.data_ptr(),
                                            lps.data_ptr() if want_logprobs else None, stamp.data_ptr(), ops.stream_ptr()), "hirest_whisper_step_tail")
    torch.cuda.synchronize()
    assert int(ids[R_]) == -7 and bool((toks[R_] == -7).all()) and bool((toks[:R_, :2 + step] == -7).all()) and bool((toks[:R_, 3 + step:] == -7).all())
    if want_logprobs:
        assert bool((lps[R_] == CANARY).all())
    st = st.cpu()
    return {"ids": ids[:R_].cpu().numpy(), "tokens": toks[:R_, 2 + step].cpu().numpy(), "state": st[:, :5].numpy(),
            "sum": st[:, 5].view(torch.float32).numpy(), "no_speech": st[:, 6].view(torch.float32).numpy(),
            "last_lp": st[:, 7].view(torch.float32).numpy(), "logprobs": lps[:R_].cpu().numpy() if want_logprobs else None, "stamp": int(stamp[0])}


def rule_histories(c):
    tb = c.timestamp_begin
    top = c.n_vocab - 1
    return {"first": [], "after_ts_only": [tb + 2], "after_closed_pair": [tb, 7, tb + 4, tb + 4], "after_text_ts": [tb, 7, 8, tb + 6],
            "last_ts_at_max_closed": [tb, 7, top, top], "last_ts_at_max_open": [tb, 7, top], "text": [tb + 1, 9, 10, 11]}


@pytest.mark.parametrize("V", [200, 51864])
def test_tail_greedy_against_restatement(V, dev):
    c = consts_for(V)
    tb = c.timestamp_begin
    hist = rule_histories(c)
    names, seqs, rows = [], [], []
    base = seeded("tail.logits", (len(hist) + 3, V), V, 3.0).numpy().astype(np.float64)
    for i, (name, seq) in enumerate(hist.items()):
        names.append(name); seqs.append(seq); rows.append(base[i])
    # the log-sum-exp rule 1e-3 above and 1e-3 below its threshold (the bars below are three orders of magnitude smaller)
    for name, delta, row in (("lse_above", 1e-3, base[len(hist)]), ("lse_below", -1e-3, base[len(hist) + 1])):
        seq = hist["text"]
        gap = R.tail_row(c, row, seq)["lse_gap"]
        row = row.copy()
        row[tb:] += delta - gap
        names.append(name); seqs.append(seq); rows.append(row)
    names.append("completed"); seqs.append(hist["text"]); rows.append(base[len(hist) + 2])
    logits = torch.from_numpy(np.stack(rows).astype(np.float32))
    completed = [n == "completed" for n in names]
    sum0 = [-0.25 * i for i in range(len(names))]
    got = tail_call(c, logits, seqs, completed, sum0, dev)
    x64 = logits.numpy().astype(np.float64)
    bar = 0.0
    refs = []
    for r, name in enumerate(names):
        ref, f32 = R.tail_row(c, x64[r], seqs[r]), R.tail_row(c, x64[r], seqs[r], np.float32)
        refs.append(ref)
        bar = max(bar, abs(float(f32["logprob"]) - ref["logprob"]), abs(float(np.float32(sum0[r]) + f32["logprob"]) - (sum0[r] + ref["logprob"])))
        if ref["no_speech_prob"] is not None:
            bar = max(bar, abs(float(f32["no_speech_prob"]) - ref["no_speech_prob"]))
    bar *= 4
    assert refs[names.index("lse_above")]["lse_gap"] > 0 > refs[names.index("lse_below")]["lse_gap"]
    assert refs[names.index("lse_above")]["suppressed"][:tb].all() and not refs[names.index("lse_below")]["suppressed"][:tb].all()
    worst = 0.0
    for r, name in enumerate(names):
        ref = refs[r]
        if name == "completed":
            assert got["ids"][r] == c.eot and got["tokens"][r] == c.eot and got["sum"][r] == np.float32(sum0[r])
            assert bool((got["logprobs"][r] == CANARY).all()) and got["state"][r].tolist() == [4, 11, 10, tb + 1, 1]
            continue
        assert np.array_equal(np.isneginf(got["logprobs"][r]), ref["suppressed"]), (name, np.flatnonzero(np.isneginf(got["logprobs"][r]) != ref["suppressed"]))
        assert ref["margin"] > bar, (name, ref["margin"])
        assert got["ids"][r] == ref["pick"] == got["tokens"][r], name
        e_lp = abs(float(got["last_lp"][r]) - ref["logprob"])
        e_sum = abs(float(got["sum"][r]) - (sum0[r] + ref["logprob"]))
        worst = max(worst, e_lp, e_sum)
        assert e_lp <= bar and e_sum <= bar, (name, e_lp, e_sum, bar)
        keep = ~ref["suppressed"]
        full = x64[r][keep] - (x64[r][keep].max() + np.log(np.exp(x64[r][keep] - x64[r][keep].max()).sum()))
        assert float(np.abs(got["logprobs"][r][keep] - full).max()) <= bar
        if name == "first":
            e_ns = abs(float(got["no_speech"][r]) - ref["no_speech_prob"])
            worst = max(worst, e_ns)
            assert e_ns <= bar
        nxt = R.advance(c, seqs[r], ref["pick"])
        if nxt is None:
            assert got["state"][r][4] == 1 and got["state"][r][0] == len(seqs[r])
        else:
            stamps = [t for t in nxt if t >= tb]
            assert got["state"][r].tolist() == [len(nxt), nxt[-1], nxt[-2] if len(nxt) > 1 else -1, stamps[-1] if stamps else -1, 0]
    print(f"tail V {V}: worst |logprob, sum, no_speech - fp64| {worst:.3e}, bar (4 x the fp32 CPU evaluation's error) {bar:.3e}")
    assert got["stamp"] == (1 << 1) | 0
    # two runs, same bits; and the stamp says done once every row is
    again = tail_call(c, logits, seqs, completed, sum0, dev)
    assert all(np.array_equal(got[k], again[k]) for k in ("ids", "sum", "no_speech", "last_lp", "logprobs"))
    done = tail_call(c, logits[:2], [hist["text"]] * 2, [True, True], [0.0, 0.0], dev, step=3)
    assert done["stamp"] == (4 << 1) | 1


def test_tail_without_rules_padding_and_eot(dev):
    """without_timestamps: only the mask and blank suppression; pad columns never win; an eot pick completes the row and counts its logprob"""
    V, n_vocab = 204, 201
    c = consts_for(200)
    c.n_vocab, c.timestamp_rules = n_vocab, False
    x = seeded("tail.nr", (3, V), 9, 2.0)
    x[:, n_vocab:] = 50.0                                              # the pad columns would win if they were looked at
    x[1, c.eot] = 20.0
    x[2, c.eot] = 20.0
    got = tail_call(c, x, [[], [4], []], [False] * 3, [0.0] * 3, dev, n_vocab=n_vocab)
    x64 = x.numpy().astype(np.float64)
    for r, seq in enumerate([[], [4], []]):
        ref = R.tail_row(c, x64[r], seq)
        assert np.array_equal(np.isneginf(got["logprobs"][r]), ref["suppressed"]) and got["ids"][r] == ref["pick"]
        assert abs(float(got["sum"][r]) - ref["logprob"]) < 1e-5
    assert got["ids"][1] == c.eot and got["state"][1].tolist() == [1, 4, -1, -1, 1]            # completed, its history frozen
    assert got["ids"][2] != c.eot and got["ids"][0] < n_vocab                                   # blank suppression held eot back at the first position
    assert abs(float(got["no_speech"][0]) - R.tail_row(c, x64[0], [])["no_speech_prob"]) < 1e-6


def test_generator_bits_equal_restatement(dev):
    out = torch.empty((5, 200), dtype=torch.int32, device=dev)
    for seed, serial in ((0, 0), (7, 3), (0xFFFFFFFF, 0xFFFFFFFF)):
        _lib.check(_lib.load().hirest_whisper_gumbel_bits(seed, serial, 5, 200, out.data_ptr(), ops.stream_ptr()), "hirest_whisper_gumbel_bits")
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.draw_bits(seed, serial, 5, 200)), (seed, serial)


@pytest.mark.parametrize("V", [200, 51864])
def test_tail_sampled_against_restatement(V, dev):
    c = consts_for(V)
    hist = rule_histories(c)
    seqs = [hist["first"], hist["after_closed_pair"], hist["after_text_ts"], hist["text"], hist["text"], hist["after_ts_only"], hist["text"],
            hist["after_closed_pair"]]
    R_, T, seed = len(seqs), 0.4, 21
    logits = seeded("tail.sampled", (R_, V), V + 1, 3.0)
    x64 = logits.numpy().astype(np.float64)
    serials = range(16 if V == 200 else 4)
    under = total = 0
    e_sum = yard_sum = 0.0
    for serial in serials:
        got = tail_call(c, logits, seqs, [False] * R_, [0.0] * R_, dev, temperature=T, seed=seed, serial=serial, want_logprobs=False)
        bits = R.draw_bits(seed, serial, R_, V)
        for r in range(R_):
            ref = R.tail_row(c, x64[r], seqs[r], np.float64, T, R.gumbel(bits[r], np.float64))
            f32 = R.tail_row(c, x64[r], seqs[r], np.float32, T, R.gumbel(bits[r], np.float32))
            keep = ~ref["suppressed"]
            s64 = x64[r][keep] / T + R.gumbel(bits[r], np.float64)[keep]
            s32 = (x64[r][keep].astype(np.float32) / np.float32(T) + R.gumbel(bits[r], np.float32)[keep]).astype(np.float64)
            bar = 4 * float(np.abs(s32 - s64).max())
            total += 1
            if ref["margin"] <= bar:
                under += 1
                continue
            assert got["ids"][r] == ref["pick"], (serial, r, got["ids"][r], ref["pick"], ref["margin"], bar)
            # the sum takes the log-probability at temperature 1
            e_sum = max(e_sum, abs(float(got["sum"][r]) - ref["logprob"]))
            yard_sum = max(yard_sum, abs(float(f32["logprob"]) - ref["logprob"]))
    print(f"tail sampled V {V}: {under} of {total} draws under the margin bar ({100.0 * under / total:.2f} %); worst |sum_logprobs - fp64| "
          f"{e_sum:.3e}, fp32 CPU evaluation {yard_sum:.3e}")
    assert under <= 0.01 * total
    assert e_sum <= 4 * yard_sum


def test_tail_draws_follow_the_softmax(dev):
    """4096 rows of the same 16 logits in one launch at T = 1: chi-square of the picks against the softmax, 15 degrees of freedom, below
    the 99.9 % quantile 37.70.  Deterministic: seed 3 gives 8.06 on the CPU restatement."""
    logits = np.linspace(-1.5, 1.5, 16)[np.argsort(np.sin(np.arange(16) * 2.1))]
    p = np.exp(logits) / np.exp(logits).sum()
    c = R.Consts(16, 15, -1, 0, 1, None, blank=-1, suppress=[], suppress_blank=False, timestamp_rules=False)
    x = torch.from_numpy(np.tile(logits.astype(np.float32), (4096, 1)))
    got = tail_call(c, x, [[1]] * 4096, [False] * 4096, [0.0] * 4096, dev, temperature=1.0, seed=3, want_logprobs=False)
    cnt = np.bincount(got["ids"], minlength=16)
    chi = float(((cnt - 4096 * p) ** 2 / (4096 * p)).sum())
    want = np.argmax(logits[None].astype(np.float32) + R.gumbel(R.draw_bits(3, 0, 4096, 16), np.float32), 1)
    print(f"tail draws: chi-square {chi:.2f} (15 dof, 99.9 % quantile 37.70); {int((want != got['ids']).sum())} of 4096 picks differ from the CPU restatement")
    assert chi < 37.70
    assert cnt.min() > 0


# ---------------------------------------------------------------------------------------------------------------- the decoder
_DECODERS = {}


def decoder(case, dev):
    """(TextDecoder on the device, xa [W, Tk, D] on the device, fixture, fp64 logits [W, T, V]): built once per case, never modified"""
    if case not in _DECODERS:
        cfg, eot, seed, windows = synth.WHISPER_DEC_CASES[case]
        sd = synth.whisper_decoder_state_dict(cfg, seed, eot, synth.WHISPER_DEC_EOT_BIAS[case])
        z = dict(np.load(os.path.join(GOLDEN, f"whisper_dec_{case}.npz")))
        emb = sd["decoder.embed_tokens.weight"].double().numpy()
        _DECODERS[case] = (whisper.TextDecoder(cfg, sd).to(dev), synth.whisper_audio_states(cfg, windows, seed + 100).to(dev), z,
                           z["hidden64"] @ emb.T, sd)
    return _DECODERS[case]


@pytest.mark.parametrize("case", ["p", "q", "r"])
def test_decoder_teacher_forced(case, dev):
    dec, xa, z, want, _ = decoder(case, dev)
    got = dec(torch.from_numpy(z["tokens"]), xa).cpu().double().numpy()
    assert got.shape == want.shape
    err, bar = float(np.abs(got - want).max()), 4 * float(z["err32"])
    print(f"decoder {case} teacher-forced: max |got - fp64| {err:.3e}, bar (4 x fp32 CPU forward) {bar:.3e}, ratio to the yardstick {4 * err / bar:.2f}")
    assert err <= bar


@pytest.mark.parametrize("case", ["p", "q", "r"])
def test_decoder_steps_through_the_cache(case, dev):
    """The same logits one position at a time through hirest_whisper_decode_step and the in-place cache — for q 5 rows over its 2 windows —
    and a row's logits do not depend on the other rows of the step."""
    dec, xa, z, want, _ = decoder(case, dev)
    tokens = torch.from_numpy(z["tokens"]).to(dev)
    W, T = tokens.shape
    rows = [0, 0, 0, 1, 1] if W == 2 else [0, 0, 0]
    kc = whisper.KVCache(dec, xa, torch.tensor(rows, dtype=torch.int32), T)
    solo = whisper.KVCache(dec, xa, torch.tensor(rows[-1:], dtype=torch.int32), T)
    err = 0.0
    for t in range(T):
        ids = tokens[rows, t].contiguous()
        logits = dec.step(ids, kc)[:, :dec.vocab].clone()
        alone = dec.step(ids[-1:].contiguous(), solo)[:, :dec.vocab]
        assert torch.equal(alone[0], logits[-1]) and torch.equal(logits[0], logits[1]), t
        got = logits.cpu().double().numpy()
        err = max(err, float(np.abs(got - want[rows, t]).max()))
    bar = 4 * float(z["err32"])
    print(f"decoder {case} step by step: max |got - fp64| {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    with pytest.raises(ValueError):
        dec.step(ids, kc)                                             # the cache is full


def test_decoder_vocabulary_that_is_no_multiple_of_four(dev):
    """A multilingual checkpoint's 51865 in small: case p with a 201st token.  The embedding is zero-padded to 204 rows, forward() returns
    201 columns, and they are case p's logits plus the new row's (the states before the LM head do not depend on an unused embedding row)."""
    _, xa, z, want, sd = decoder("p", dev)
    cfg = {**synth.WHISPER_DEC_CASES["p"][0], "vocab_size": 201}
    extra = seeded("dec.row201", (1, cfg["d_model"]), 5, 0.1)
    sd201 = {**sd, "decoder.embed_tokens.weight": torch.cat([sd["decoder.embed_tokens.weight"], extra], 0)}
    dec = whisper.TextDecoder(cfg, sd201).to(dev)
    assert dec.vocab_padded == 204
    got = dec(torch.from_numpy(z["tokens"]), xa).cpu().double().numpy()
    assert got.shape == want.shape[:2] + (201,)
    full = np.concatenate([want, z["hidden64"] @ extra.double().numpy().T], axis=-1)
    assert float(np.abs(got - full).max()) <= 4 * float(z["err32"])
    kc = whisper.KVCache(dec, xa, torch.zeros(2, dtype=torch.int32), 4)
    logits = dec.step(torch.from_numpy(z["tokens"][0, :1]).to(dev).expand(2).contiguous(), kc)
    assert logits.shape == (2, 204) and bool((logits[:, 201:] == 0).all())                      # the pad columns: zero rows of the head
    assert float(np.abs(logits[0, :201].cpu().double().numpy() - full[0, 0]).max()) <= 4 * float(z["err32"])


def model_for(case, dev, enc_cfg=None):
    cfg, eot, seed, _ = synth.WHISPER_DEC_CASES[case]
    cfg = {**cfg, **(enc_cfg or {})}
    enc = synth.whisper_encoder_state_dict(cfg, 73)
    sd = {**{"encoder." + k: v for k, v in enc.items()}, **synth.whisper_decoder_state_dict(cfg, seed, eot, synth.WHISPER_DEC_EOT_BIAS[case])}
    return whisper.Whisper(cfg, sd, synth.whisper_tokenizer(eot)).to(dev)


_MODELS = {}


@pytest.mark.parametrize("without_timestamps", [False, True])
@pytest.mark.parametrize("has_prompt", [False, True])
@pytest.mark.parametrize("case", ["p", "q"])
def test_greedy_decode_equals_fixture(case, has_prompt, without_timestamps, dev):
    if case not in _MODELS:
        _MODELS[case] = model_for(case, dev)
    model = _MODELS[case]
    _, xa, z, _, _ = decoder(case, dev)
    key = f"greedy_{int(has_prompt)}{int(without_timestamps)}"
    want, (avg, nsp, err32, margin) = z[key + "_tokens"].tolist(), z[key + "_stats"]
    opts = whisper.DecodingOptions(temperature=0.0, prompt=z["prompt9"].tolist() if has_prompt else None, without_timestamps=without_timestamps)
    res = whisper.decode(model, xa[0], opts)
    print(f"greedy {case} prompt={has_prompt} without_timestamps={without_timestamps}: {len(res.tokens)} tokens, avg_logprob {res.avg_logprob:.6f} "
          f"(fp64 {avg:.6f}), no_speech {res.no_speech_prob:.3e} (fp64 {nsp:.3e}), fixture's smallest margin {margin:.2e}")
    assert res.tokens == want
    bar = 4 * err32
    assert abs(res.avg_logprob - avg) <= bar and abs(res.no_speech_prob - nsp) <= bar
    assert res.temperature == 0.0 and res.text == model.tokenizer.decode(want).strip()


def test_sampled_decode(dev):
    if "q" not in _MODELS:
        _MODELS["q"] = model_for("q", dev)
    model = _MODELS["q"]
    cfg, eot, _, _ = synth.WHISPER_DEC_CASES["q"]
    _, xa, _, _, _ = decoder("q", dev)
    opts = whisper.DecodingOptions(temperature=0.4, best_of=5, seed=5)
    res, cands = whisper.decode(model, xa[1], opts, return_candidates=True)
    res2, cands2 = whisper.decode(model, xa[1], opts, return_candidates=True)
    assert cands == cands2 and res.tokens == res2.tokens and res.avg_logprob == res2.avg_logprob          # deterministic for a seed
    other, _ = whisper.decode(model, xa[1], whisper.DecodingOptions(temperature=0.4, best_of=5, seed=6), return_candidates=True)
    assert len(cands) == 5 and len({tuple(t) for t, _ in cands}) > 1                                      # not five copies
    scores = [lp / max(len(t), 1) for t, lp in cands]
    assert res.tokens == cands[int(np.argmax(scores))][0]
    assert res.avg_logprob == pytest.approx(max(zip(scores, cands))[1][1] / (len(res.tokens) + 1))
    k = synth.whisper_tail_consts(cfg, eot)
    c = R.Consts(k["n_vocab"], k["eot"], k["no_speech"], k["no_timestamps"], k["timestamp_begin"], k["max_initial_timestamp_index"], k["blank"],
                 k["suppress"])
    for t, lp in cands:
        assert R.grammar_ok(c, t) and not set(t) & set(k["suppress"]) and lp < 0, t
    print(f"sampled q: lengths {[len(t) for t, _ in cands]}, scores {[round(s, 3) for s in scores]}; seed 6 gives {len(other.tokens)} tokens")


def test_transcribe_end_to_end(dev, tmp_path):
    """31 s of synthetic audio through the case-p decoder behind the 1500-position encoder: real 3000-frame windows, well-formed segments, an
    .srt that parses, and a second run that is identical.  The weights are synthetic: what the segments say is not asserted."""
    model = model_for("p", dev, synth.WHISPER_E2E)
    audio = synth.audio_clip("mixed", 31 * 16000, 71)
    path = str(tmp_path / "clip.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(audio, -1, 1 - 1 / 32768) * 32768).astype("<i2").tobytes())
    kw = dict(temperature=(0.0, 0.4), best_of=5, beam_size=None, compression_ratio_threshold=2.4, logprob_threshold=-1.0, no_speech_threshold=0.6)
    out = whisper.transcribe(model, path, **kw)
    segs = out["segments"]
    print(f"transcribe: {len(segs)} segments, seeks {sorted({s['seek'] for s in segs})}, temperatures {sorted({s['temperature'] for s in segs})}")
    assert out["language"] == "en" and [s["id"] for s in segs] == list(range(len(segs)))
    assert all(s["start"] <= s["end"] for s in segs)
    assert all(a["start"] <= b["start"] and a["seek"] <= b["seek"] for a, b in zip(segs, segs[1:]))
    assert all(0 <= s["seek"] < 3100 and s["end"] <= 61.0 for s in segs)
    srt = tmp_path / "clip.srt"
    with open(srt, "w", encoding="utf-8") as f:
        whisper.utils.write_srt(segs, file=f)
    spans = dataset.read_srt_spans(srt.read_text(encoding="utf-8"))
    assert spans == [(int(round(s["start"] * 1000)) // 1000, int(round(s["end"] * 1000)) // 1000) for s in segs]
    again = whisper.transcribe(model, path, **kw)
    assert again["text"] == out["text"] and [(s["tokens"], s["avg_logprob"]) for s in again["segments"]] == [(s["tokens"], s["avg_logprob"]) for s in segs]
