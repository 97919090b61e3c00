"""The ragged multi-window prefill on the device (csrc/whisper_prefill.hip).  The yardstick of every piece is the
per-window path it replaces in the decoding loop, bit for bit: hirest_attention_f32_qkv at B = 1 for the two ragged attention forms,
TextDecoder.prefill(tokens[1, T], kc, rows=, window=) for the caches and the logits, tests/_whisper_lockstep.py for decode_many().
Against fp64 the bars are the project's standing one — 4 x the error of the same formula evaluated in fp32 on the CPU — and, for the
whole prefill, the fp64 fixtures of tests/golden/whisper_dec_{p,q,s}.npz as tests/test_gpu_whisper_dec.py holds the single-window path.

Measured on an MI355X (printed by the tests; the bars are the yardsticks above, not these numbers):
    ragged causal self-attention  max |got - fp64| 8.4e-7, fp32 CPU formula 7.2e-7 (ratio 1.16, bar 4)
    ragged cross-attention        Tk 33 6.6e-7 / 5.0e-7 (1.31), Tk 70 6.2e-7 / 4.4e-7 (1.40), Tk 261 6.6e-7 / 4.6e-7 (1.42)
    prefill_many, logits_last     p 1.1e-6 (bar 6.9e-6), q 8.4e-7 (bar 7.0e-6), s 9.6e-6 (bar 5.9e-5)
    forward over two windows, then a step  9.8e-7 (bar 7.0e-6)

"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_whisper_dec as S
from _whisper_lockstep import lockstep_decode
from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

CANARY = S.CANARY
PENALTY = -1.0e30


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def table(lengths, windows=None, first_rows=None, groups=None):
    """sequences packed in the given order -> (the C array, offsets)"""
    n = len(lengths)
    offs = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    seqs = [(offs[i], lengths[i], windows[i] if windows else 0, first_rows[i] if first_rows else i, groups[i] if groups else 1, -1) for i in range(n)]
    return whisper._seq_table(seqs), offs


def attention_ref(q, k, v, causal, dtype):
    """softmax(q k^T / 8 (+ PENALTY where key > query)) v per head in ``dtype``: q [Tq, H, 64], k / v [Tk, H, 64] -> [Tq, H, 64]"""
    q, k, v = (a.astype(dtype) for a in (q, k, v))
    s = np.einsum("qhd,khd->hqk", q, k) * dtype(0.125)
    if causal:
        s = s + np.where(np.arange(k.shape[0])[None, :] > np.arange(q.shape[0])[:, None], dtype(PENALTY), dtype(0.0))[None]
    p = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("hqk,khd->qhd", p / p.sum(-1, keepdims=True), v)


def qkv_attention(q, ldq, k, v, ldkv, T, Tk, H, causal, dev):
    """hirest_attention_f32_qkv at B = 1 on device operands given by address -> [T, H * 64] on the device"""
    out = torch.empty((T, H * 64), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().hirest_attention_f32_qkv(q, ldq, k, v, ldkv, out.data_ptr(), 1, T, Tk, H, 64, 0.125, 0.0, PENALTY if causal else 0.0,
                                                    ops.stream_ptr()), "hirest_attention_f32_qkv")
    return out


# ---------------------------------------------------------------------------------------------------------------- ragged self-attention
LENGTHS = [1, 2, 31, 32, 33, 64, 65, 97]          # one-wave and multi-wave blocks, the 32-key tile edges, a sequence of one token


def run_causal(qkv, lengths, H, dev):
    """packed q | k | v rows [N, 3 D] on the device -> [N, D]; the output sits in a canary-filled buffer with a row behind it"""
    N, D = qkv.shape[0], H * 64
    t, _ = table(lengths)
    out = torch.full((N + 1, D), CANARY, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().hirest_attention_f32_varlen_causal(qkv.data_ptr(), 3 * D, qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, out.data_ptr(),
                                                              t, len(lengths), H, 0.125, 0.0, PENALTY, ops.stream_ptr()),
               "hirest_attention_f32_varlen_causal")
    torch.cuda.synchronize()
    assert bool((out[N] == CANARY).all()), "the output was written behind its rows"
    return out[:N]


def test_ragged_causal_self_attention(dev):
    H, D = 2, 128
    offs = np.concatenate([[0], np.cumsum(LENGTHS)]).tolist()
    N = offs[-1]
    host = S.seeded("prefill.qkv", (N, 3 * D), 31, 2.0)
    qkv = host.to(dev)
    got = run_causal(qkv, LENGTHS, H, dev)
    err = yard = 0.0
    want = []
    for i, T in enumerate(LENGTHS):
        base = qkv.data_ptr() + 4 * offs[i] * 3 * D
        want.append(qkv_attention(base, 3 * D, base + 4 * D, base + 8 * D, 3 * D, T, T, H, True, dev))
        assert torch.equal(got[offs[i]:offs[i + 1]], want[i]), T
        rows = host[offs[i]:offs[i + 1]].numpy().reshape(T, 3, H, 64)
        ref = attention_ref(rows[:, 0], rows[:, 1], rows[:, 2], True, np.float64)
        f32 = attention_ref(rows[:, 0], rows[:, 1], rows[:, 2], True, np.float32)
        err = max(err, float(np.abs(want[i].cpu().numpy().reshape(T, H, 64).astype(np.float64) - ref).max()))
        yard = max(yard, float(np.abs(f32.astype(np.float64) - ref).max()))
        # the sequence alone in a call
        assert torch.equal(run_causal(qkv[offs[i]:offs[i + 1]].contiguous(), [T], H, dev), want[i]), T
    print(f"ragged causal self-attention: max |got - fp64| {err:.3e}, fp32 CPU formula {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 4 * yard
    # the same sequences packed in another order, and a second run of the first
    order = [5, 0, 7, 2, 6, 1, 4, 3]
    shuffled = torch.cat([qkv[offs[i]:offs[i + 1]] for i in order]).contiguous()
    out = run_causal(shuffled, [LENGTHS[i] for i in order], H, dev)
    at = 0
    for i in order:
        assert torch.equal(out[at:at + LENGTHS[i]], want[i]), i
        at += LENGTHS[i]
    assert torch.equal(run_causal(qkv, LENGTHS, H, dev), got)


# ---------------------------------------------------------------------------------------------------------------- ragged cross-attention
@pytest.mark.parametrize("Tk", [33, 70, 261])
def test_ragged_cross_attention(Tk, dev):
    H, D = 2, 128
    lengths, windows = [1, 5, 33, 65], [2, 0, 0, 1]
    t, offs = table(lengths, windows)
    N = offs[-1]
    q_host, kv_host = S.seeded("prefill.xq", (N, D), 5 * Tk, 3.0), S.seeded("prefill.xkv", (3, Tk, 2 * D), 7 * Tk, 1.5)
    q, kv = q_host.to(dev), kv_host.to(dev)
    out = torch.full((N + 1, D), CANARY, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().hirest_attention_f32_varlen_cross(q.data_ptr(), D, kv.data_ptr(), 2 * D, Tk * 2 * D, 3, Tk, out.data_ptr(), t, len(lengths), H,
                                                             0.125, 0.0, ops.stream_ptr()), "hirest_attention_f32_varlen_cross")
    torch.cuda.synchronize()
    assert bool((out[N] == CANARY).all())
    err = yard = 0.0
    for i, (T, w) in enumerate(zip(lengths, windows)):
        want = qkv_attention(q.data_ptr() + 4 * offs[i] * D, D, kv[w].data_ptr(), kv[w].data_ptr() + 4 * D, 2 * D, T, Tk, H, False, dev)
        assert torch.equal(out[offs[i]:offs[i + 1]], want), (T, w)
        qs = q_host[offs[i]:offs[i + 1]].numpy().reshape(T, H, 64)
        k, v = kv_host[w, :, :D].numpy().reshape(Tk, H, 64), kv_host[w, :, D:].numpy().reshape(Tk, H, 64)
        ref, f32 = attention_ref(qs, k, v, False, np.float64), attention_ref(qs, k, v, False, np.float32)
        err = max(err, float(np.abs(want.cpu().numpy().reshape(T, H, 64).astype(np.float64) - ref).max()))
        yard = max(yard, float(np.abs(f32.astype(np.float64) - ref).max()))
    print(f"ragged cross-attention Tk {Tk}: max |got - fp64| {err:.3e}, fp32 CPU formula {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 4 * yard


# ---------------------------------------------------------------------------------------------------------------- scatter
def test_scatter_writes_its_positions_and_nothing_else(dev):
    D, T_max, R = 128, 12, 10
    lengths, groups, first_rows = [4, 1, 9], [1, 5, 3], [0, 1, 7]                 # row 6 lies between two ranges and belongs to nobody
    t, offs = table(lengths, None, first_rows, groups)
    src = S.seeded("prefill.scatter", (offs[-1], 3 * D), 3).to(dev)
    ck = torch.full((R + 1, T_max, D), CANARY, dtype=torch.float32, device=dev)
    cv = torch.full((R + 1, T_max, D), CANARY, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().hirest_whisper_prefill_scatter(src.data_ptr() + 4 * D, src.data_ptr() + 8 * D, 3 * D, ck.data_ptr(), cv.data_ptr(), R, T_max, D,
                                                          t, 3, ops.stream_ptr()), "hirest_whisper_prefill_scatter")
    torch.cuda.synchronize()
    want_k, want_v = torch.full_like(ck, CANARY), torch.full_like(cv, CANARY)
    for i, (T, g, r0) in enumerate(zip(lengths, groups, first_rows)):
        want_k[r0:r0 + g, :T] = src[offs[i]:offs[i + 1], D:2 * D]
        want_v[r0:r0 + g, :T] = src[offs[i]:offs[i + 1], 2 * D:]
    assert torch.equal(ck, want_k) and torch.equal(cv, want_v)
    assert bool((ck[6] == CANARY).all()) and bool((ck[R] == CANARY).all()) and bool((ck[0, 4:] == CANARY).all()) and bool((cv[7:10, 9:] == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------- the whole prefill
_LONG = {}


def long_decoder(dev):
    """WHISPER_DEC_LONG's decoder, audio states and state dict (no fixture: its yardstick is the per-window path)"""
    if not _LONG:
        cfg, eot, seed, windows = synth.WHISPER_DEC_LONG
        sd = synth.whisper_decoder_state_dict(cfg, seed, eot, 0.0)
        _LONG["v"] = (whisper.TextDecoder(cfg, sd).to(dev), synth.whisper_audio_states(cfg, windows, seed + 100).to(dev), sd)
    return _LONG["v"]


def ragged_prompts(case, eot, ctx):
    """(prompts, sot indices): a bare <|startoftranscript|>; one that fills the context; <|startofprev|> + 9 tokens + sot +
    <|notimestamps|>, whose sot is not its last position; for the long context also 65 and 130 tokens"""
    sp = synth.whisper_special_tokens(eot)
    sot, prev, nots = sp["<|startoftranscript|>"], sp["<|startofprev|>"], sp["<|notimestamps|>"]
    text = synth.token_ids(f"prefill.{case}", 2 * ctx + 200, eot, 17).tolist()
    prompts = [[sot], [prev] + text[:ctx - 2] + [sot], [prev] + text[ctx:ctx + 9] + [sot, nots]]
    sots = [0, ctx - 1, 10]
    if ctx >= 130:
        prompts += [[prev] + text[200:263] + [sot], [prev] + text[210:337] + [sot, nots]]
        sots += [64, 128]
        assert [len(p) for p in prompts[3:]] == [65, 130]
    assert [len(p) for p in prompts[:3]] == [1, ctx, 12] and all(p[i] == sot for p, i in zip(prompts, sots))
    return prompts, sots


def canary_cache(dec, xa, row_window, T_max):
    kc = whisper.KVCache(dec, xa, torch.tensor(row_window, dtype=torch.int32), T_max, per_row=True)
    for t in kc.self_k + kc.self_v:
        t.fill_(CANARY)
    return kc


@pytest.mark.parametrize("case", ["p", "q", "s", "long"])
def test_prefill_many_equals_the_per_window_prefill(case, dev):
    if case == "long":
        dec, xa, _ = long_decoder(dev)
        eot, z, want64 = synth.WHISPER_DEC_LONG[1], None, None
    else:
        dec, xa, z, want64, _ = S.decoder(case, dev)
        eot = synth.WHISPER_DEC_CASES[case][1]
    W, ctx, Vp = int(xa.shape[0]), dec.ctx, dec.vocab_padded
    prompts, sots = ragged_prompts(case, eot, ctx)
    n = len(prompts)
    groups = [1, 5, 3, 2, 1][:n]
    windows = [[0] * 5, [0, 1, 1, 0, 1], [0, 2, 2, 1, 0]][W - 1][:n]                # two sequences on one window wherever there are two
    first_rows, r = [], 0
    for i, g in enumerate(groups):
        r += 1 if i == 2 else 0                                        # a spare row in front of the third range
        first_rows.append(r)
        r += g
    R = r + 1                                                          # and one behind the last
    row_window = [0] * R
    for r0, g, w in zip(first_rows, groups, windows):
        row_window[r0:r0 + g] = [w] * g
    # the yardstick: each prompt through the single-window form into its rows of a canary-filled cache
    ref = canary_cache(dec, xa, row_window, ctx)
    want_last, want_sot = [], []
    for p, s, r0, g, w in zip(prompts, sots, first_rows, groups, windows):
        logits = dec.prefill(torch.tensor([p], dtype=torch.int32), ref, rows=slice(r0, r0 + g), window=w)
        want_last.append(logits[len(p) - 1].clone())
        want_sot.append(logits[s].clone())
    for order in (list(range(n)), list(range(n))[::-1], [1, 0, 2, 4, 3][:n] if n > 3 else [1, 0, 2]):
        kc = canary_cache(dec, xa, row_window, ctx)
        pick = lambda v: [v[i] for i in order]
        last, at_sot = dec.prefill_many(pick(prompts), kc, pick(first_rows), pick(groups), pick(windows), pick(sots))
        torch.cuda.synchronize()
        assert last.shape == (n, Vp) and at_sot.shape == (n, Vp)
        for k, i in enumerate(order):
            T = len(prompts[i])
            assert torch.equal(last[k], want_last[i]), (case, order, i)
            if sots[i] != T - 1:
                assert torch.equal(at_sot[k], want_sot[i]), (case, order, i)
        for i in range(dec.layers):
            assert torch.equal(kc.self_k[i], ref.self_k[i]) and torch.equal(kc.self_v[i], ref.self_v[i]), (case, order, i)
        # (equal to a cache that was canary everywhere the single-window form did not write; said once more for what matters most)
        for r0, g, p in zip(first_rows, groups, prompts):
            assert bool((kc.self_k[0][r0:r0 + g, len(p):] == CANARY).all()) and bool((kc.self_v[0][r0:r0 + g, :len(p)] != CANARY).all())
        assert bool((kc.self_k[0][first_rows[2] - 1] == CANARY).all()) and bool((kc.self_v[-1][R - 1] == CANARY).all())
    # a prompt alone in a call, and no sot row asked for: logits_sot is None then
    kc = canary_cache(dec, xa, row_window, ctx)
    last, none = dec.prefill_many(prompts[2:3], kc, first_rows[2:3], groups[2:3], windows[2:3])
    assert none is None and torch.equal(last[0], want_last[2])
    r0, g = first_rows[2], groups[2]
    assert torch.equal(kc.self_k[0][r0:r0 + g], ref.self_k[0][r0:r0 + g]) and bool((kc.self_k[0][:r0] == CANARY).all())
    # the 4096-row split: the same prompts through consecutive calls of at most ctx packed rows
    kc = canary_cache(dec, xa, row_window, ctx)
    assert len(whisper.prefill_plan(prompts, first_rows, groups, windows, sots, ctx)) >= 2
    last, at_sot = dec.prefill_many(prompts, kc, first_rows, groups, windows, sots, rows_per_call=ctx)
    assert all(torch.equal(last[i], want_last[i]) for i in range(n)) and torch.equal(at_sot[2], want_sot[2])
    assert all(torch.equal(kc.self_k[i], ref.self_k[i]) and torch.equal(kc.self_v[i], ref.self_v[i]) for i in range(dec.layers))
    if z is None:
        return
    # the teacher-forced fp64 fixture: every window's sequence in one call, the last position's logits to 4 x err32
    tokens = z["tokens"]
    T = tokens.shape[1]
    kc = canary_cache(dec, xa, list(range(W)), T)
    last, _ = dec.prefill_many([tokens[w].tolist() for w in range(W)], kc, list(range(W)), [1] * W, list(range(W)))
    err, bar = float(np.abs(last[:, :dec.vocab].cpu().double().numpy() - want64[:, T - 1]).max()), 4 * float(z["err32"])
    print(f"prefill_many {case}: max |logits_last - fp64| {err:.3e}, bar (4 x fp32 CPU forward) {bar:.3e}, ratio to the yardstick {4 * err / bar:.2f}")
    assert err <= bar


def test_prefill_many_past_256_packed_rows_at_small_en_width(dev):
    """Bit equality rests on hirest_gemm_f32 giving the same bits at M = T_s and at M = N.  Case s (768 wide, MLP 3072) with twelve
    prompts of 24 tokens is 288 packed rows: the layer's products leave the <= 256-row kernels for the 64 x 64 tiles — fc2 (K = 3072)
    in their split form, through the call's own scratch — while every per-window prefill stays at 24 rows."""
    dec, xa, _, _, _ = S.decoder("s", dev)
    eot, ctx, lib = synth.WHISPER_DEC_CASES["s"][1], dec.ctx, _lib.load()
    sot = synth.whisper_special_tokens(eot)["<|startoftranscript|>"]
    text = synth.token_ids("prefill.s.rows", 12 * (ctx - 1), eot, 23).reshape(12, ctx - 1).tolist()
    prompts = [t + [sot] for t in text]
    windows = [i % 3 for i in range(12)]
    names = {}
    for M in (ctx, 12 * ctx):
        for what, (N, K) in {"qkv": (2304, 768), "fc2": (768, 3072)}.items():
            buf = C.create_string_buffer(64)
            q = _lib.GemmF32Query.make("ws", M, N, K, cus=0, select_kernel=-1, ring_mode=-1, rows_ln_mode=-1, has_workspace=1)
            assert lib.hirest_gemm_f32_dispatch_name(C.byref(q), buf, 64) == 0
            names[what, M] = buf.value.decode()
    print("dispatch:", names)
    assert all(names[w, ctx].startswith("m16<") and not names[w, 12 * ctx].startswith("m16") for w in ("qkv", "fc2")), names
    assert lib.hirest_gemm_f32_workspace_bytes(12 * ctx, 768, 3072) > 0
    ref, kc = canary_cache(dec, xa, windows, ctx), canary_cache(dec, xa, windows, ctx)
    want = [dec.prefill(torch.tensor([p], dtype=torch.int32), ref, rows=slice(i, i + 1), window=windows[i])[ctx - 1].clone()
            for i, p in enumerate(prompts)]
    last, none = dec.prefill_many(prompts, kc, list(range(12)), [1] * 12, windows)
    torch.cuda.synchronize()
    assert none is None and all(torch.equal(last[i], want[i]) for i in range(12))
    assert all(torch.equal(a, b) for a, b in zip(kc.self_k + kc.self_v, ref.self_k + ref.self_v))


# ---------------------------------------------------------------------------------------------------------------- public surface
def test_forward_with_a_cache_over_two_windows(dev):
    """Whisper's batched decoder(tokens[B, T], xa[B], kv_cache): the logits of forward(tokens, xa) row for row, and a cache that step()
    continues from.  (NotImplementedError before the multi-window prefill existed.)"""
    dec, xa, z, want64, _ = S.decoder("q", dev)
    tokens = torch.from_numpy(z["tokens"])
    W, T = tokens.shape
    assert W == 2
    rows = [0, 0, 0, 1, 1]
    kc = whisper.KVCache(dec, xa, torch.tensor(rows, dtype=torch.int32), T)
    for t in kc.self_k + kc.self_v:
        t.fill_(CANARY)
    got = dec(tokens[:, :T - 1], None, kv_cache=kc)
    want = dec(tokens[:, :T - 1], xa)
    assert got.shape == (2, T - 1, dec.vocab) and torch.equal(got, want) and kc.length == T - 1
    assert bool((kc.self_k[0][:, T - 1:] == CANARY).all()) and bool((kc.self_v[-1][:, :T - 1] != CANARY).all())
    # the same cache filled window by window through the single-window form
    ref = whisper.KVCache(dec, xa, torch.tensor(rows, dtype=torch.int32), T)
    for t in ref.self_k + ref.self_v:
        t.fill_(CANARY)
    dec.prefill(tokens[0:1, :T - 1], ref, rows=slice(0, 3), window=0)
    dec.prefill(tokens[1:2, :T - 1], ref, rows=slice(3, 5), window=1)
    ref.length = T - 1
    assert all(torch.equal(a, b) for a, b in zip(kc.self_k + kc.self_v, ref.self_k + ref.self_v))
    ids = tokens[rows, T - 1].to(dev).contiguous()
    logits = dec(ids[:, None], None, kv_cache=kc)[:, 0]
    assert torch.equal(logits, dec.step(ids, ref)[:, :dec.vocab]) and kc.length == T
    err, bar = float(np.abs(logits.cpu().double().numpy() - want64[rows, T - 1]).max()), 4 * float(z["err32"])
    print(f"forward over two windows, then a step: max |got - fp64| {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    with pytest.raises(ValueError):
        dec(tokens[:1, :3], None, kv_cache=whisper.KVCache(dec, xa, torch.tensor(rows, dtype=torch.int32), T))       # one prompt for two windows
    with pytest.raises(ValueError):
        dec.prefill(tokens[:, :3], whisper.KVCache(dec, xa, torch.tensor([0, 1, 0], dtype=torch.int32), T))         # window 0's rows apart


# ---------------------------------------------------------------------------------------------------------------- end to end
def check_decode_many(model, windows, opts):
    res, cands = whisper.decode_many(model, windows, opts, return_candidates=True)
    for k, (w, o) in enumerate(zip(windows, opts)):
        want, nsp = lockstep_decode(model, w, o)
        assert cands[k] == want, (k, cands[k], want)                                       # tokens and sum_logprobs of every candidate
        best = max(range(len(want)), key=lambda g: (want[g][1] / max(len(want[g][0]), 1), -g))
        t, lp = want[best]
        assert res[k].tokens == t and res[k].avg_logprob == lp / (len(t) + 1) and res[k].no_speech_prob == nsp, (k, res[k], want[best], nsp)
    return res


def test_decode_many_with_ragged_prompts_equals_the_lockstep_loop(dev):
    if "q" not in S._MODELS:
        S._MODELS["q"] = S.model_for("q", dev)
    m = S._MODELS["q"]
    _, xa, z, _, _ = S.decoder("q", dev)
    prompt9 = z["prompt9"].tolist()
    prompt23 = (prompt9 * 3)[:23]                                      # sot_prev + 23 + sot: the longest prompt a context of 48 admits
    windows = [xa[0], xa[1], xa[0], xa[1]]
    for without_timestamps in (False, True):                           # True: <|notimestamps|> follows sot, so sot is not the last position
        o = lambda **kw: whisper.DecodingOptions(without_timestamps=without_timestamps, **kw)
        opts = [o(temperature=0.0), o(temperature=0.4, best_of=5, seed=5, prompt=prompt23), o(temperature=0.0, prompt=prompt9),
                o(temperature=0.7, best_of=3, seed=9)]
        lens = [len(whisper._initial_tokens(m.tokenizer, x, 48)[0]) for x in opts]
        assert lens == [1 + without_timestamps, 25 + without_timestamps, 11 + without_timestamps, 1 + without_timestamps]
        res = check_decode_many(m, windows, opts)
        assert len({tuple(r.tokens) for r in res}) > 1


def test_decode_many_with_prompts_past_one_attention_block(dev):
    """the long context: initial tokens of 1, 81 (sot_prev + 79 + sot: two one-wave blocks would not hold them) and 11 in one loop"""
    cfg, eot, seed, _ = synth.WHISPER_DEC_LONG
    dec, xa, sd = long_decoder(dev)
    enc = synth.whisper_encoder_state_dict(cfg, 73)
    m = whisper.Whisper(cfg, {**{"encoder." + k: v for k, v in enc.items()}, **sd}, synth.whisper_tokenizer(eot)).to(dev)
    text = synth.token_ids("prefill.long.e2e", 200, eot, 5).tolist()
    o = lambda **kw: whisper.DecodingOptions(sample_len=12, **kw)
    opts = [o(temperature=0.0), o(temperature=0.0, prompt=text[:100]), o(temperature=0.5, best_of=3, seed=2, prompt=text[100:109])]
    assert [len(whisper._initial_tokens(m.tokenizer, x, 160)[0]) for x in opts] == [1, 81, 11]
    check_decode_many(m, [xa[0], xa[1], xa[2]], opts)
