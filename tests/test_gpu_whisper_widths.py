"""The Whisper text decoder at the widths of the released checkpoints and at the row counts production runs it with: small.en's width
(case s of hirest_amd.synth: 768 wide, 12 heads, 8200 LM-head columns) with 1 to 256 rows in a step, the per-row form of the step at 40
rows, tiny's / base's / medium's / large's widths and head counts (w384, w512, w1024, w1280), and decode() / decode_many() at 768.

Two bars throughout.  Against transformers' WhisperDecoder in fp64 (tests/golden/whisper_dec_*.npz): max |logits - fp64| <= 4 x the
error of the same forward in fp32 on the CPU, the project's bar.  Between row counts: torch.equal — decode_many == decode and
transcribe_many == transcribe rest on a row's logits being the same bits whatever kernel family the row count selects, and the exact
tests of the fp32 GEMMs (integer operands: every summation order gives the same sum) cannot show that.  Each test first asks
hirest_gemm_f32_dispatch_name which kernel every call of the step gets and asserts the families it means to run
(_whisper_dec_ref.check_small_en_step_families; tests/test_whisper_dec_host.py asserts the same at 256 CUs without a GPU).

Kernels per step at width 768 (qkv = fc1 | cross-q | out-projections | fc2 | LM head), as hirest_gemm_f32_dispatch_name names them:
    R 1 .. 32     m16ln<3,1,2> | m16ln<3,1,2> | m16<1,1,8> | m16<1,1,8> | m16ln_stream<3,1,8,0> (R 1), <3,1,8,1> (5), <3,1,8,5> (16),
                  <3,2,4,3> (17), <3,2,2,5> (32)
    R 33 .. 256   rows<mt=1,ln,mode=2> | m16ln<3,1,2> | m16<2,1,6> | m16<1,1,4> | hirest_layernorm + rows<mt=1> (R 33, 47, 48, 80),
                  rows<mt=2> (96), tile64 (256)
Widths: 512 m16ln<2,1,2> and 1024 m16ln<4,1,2> for every LayerNorm GEMM; 384 and 1280 are refused by the ln entry and take
hirest_layernorm + m16<1,1,8> / m16<1,1,3> (3 rows) or m16<2,1,6> (40 rows); fc2 is m16<1,1,4> at 40 rows from width 512 on (K >= 2048).

Measured on an MI355X (printed by the tests; the bars are the yardsticks above, not these numbers), max |got - fp64| / the fp32 CPU
forward's error (bar 4):
    s, a step of R rows     0.82 at every R of 1, 5, 16, 17, 32, 33, 47, 48, 80, 96, 256 (1.223e-05 against 1.483e-05): every row has
                            the bits of the row alone, so the figure cannot differ; the per-row form at 40 rows the same
    w384 / w512 / w1024 / w1280   teacher-forced 0.68 / 1.43 / 2.11 / 1.29, stepped through the cache 0.76 / 1.48 / 2.01 / 1.34; 40 rows
                            equal 3 rows bit for bit at all four
    s, decode()             the fixture's 8 tokens, avg_logprob -2.429613 (fp64 -2.429612), no_speech_prob 1.073e-05 (fp64 1.073e-05);
                            decode_many of 9 windows x 5 candidates equals 9 lock-step loops of 5 rows (tests/_whisper_lockstep.py)
No bit differed between the kernel families: nothing in the kernels had to change.  
"""
import numpy as np
import pytest
import torch

import _whisper_dec_ref as R
import test_gpu_whisper_dec as S
from _whisper_lockstep import lockstep_decode
from test_gpu_whisper_many import same_result
from hirest_amd import synth, whisper

pytestmark = pytest.mark.gpu

CANARY = S.CANARY
WINDOW_OF_ROW = [0, 2, 1, 1, 0, 2, 2]                                  # repeated over the rows: neighbours differ, 7 is coprime to 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


_SOLO = {}


def solo(case, dev):
    """(logits [T, W, vocab] of every window of the case stepped alone through a cache of one row, fp64 logits [W, T, vocab] on the
    device): computed once, never modified"""
    if case not in _SOLO:
        dec, xa, z, want, _ = S.decoder(case, dev)
        tokens = torch.from_numpy(z["tokens"]).to(dev)
        W, T = tokens.shape
        out = torch.empty((T, W, dec.vocab), dtype=torch.float32, device=dev)
        for w in range(W):
            kc = whisper.KVCache(dec, xa, torch.tensor([w], dtype=torch.int32), T)
            for t in range(T):
                out[t, w] = dec.step(tokens[w:w + 1, t].contiguous(), kc)[0, :dec.vocab]
        _SOLO[case] = (out, torch.from_numpy(want).to(dev))
    return _SOLO[case]


def step_names(dec, rows):
    return R.step_dispatch(rows, dec.width, dec.ffn, dec.vocab_padded)


@pytest.mark.parametrize("rows", R.STEP_ROW_COUNTS)
def test_step_rows_at_small_en_width(rows, dev):
    dec, xa, z, _, _ = S.decoder("s", dev)
    alone, want = solo("s", dev)
    names = step_names(dec, rows)
    R.check_small_en_step_families(rows, names)
    tokens = torch.from_numpy(z["tokens"]).to(dev)
    T = tokens.shape[1]
    window = torch.tensor([WINDOW_OF_ROW[r % len(WINDOW_OF_ROW)] for r in range(rows)], dtype=torch.int64, device=dev)
    kc = whisper.KVCache(dec, xa, window.to(torch.int32), T)
    err = 0.0
    for t in range(T):
        logits = dec.step(tokens[window, t].contiguous(), kc)[:, :dec.vocab]
        err = max(err, float((logits.double() - want[window, t]).abs().max()))
        same = (logits == alone[t][window]).all(dim=1)
        assert bool(same.all()), (rows, t, "rows whose bits differ from the row alone:", torch.nonzero(~same).view(-1).tolist()[:8],
                                  float((logits - alone[t][window]).abs().max()))
    yard = float(z["err32"])
    print(f"step s R {rows}: max |got - fp64| {err:.3e}, fp32 CPU forward {yard:.3e}, ratio {err / yard:.2f} (bar 4); kernels "
          f"{ {k: v[1] for k, v in names.items() if not k.endswith('_fused')} }")
    assert err <= 4 * yard


def test_step_per_row_form_at_small_en_width(dev):
    """hirest_whisper_decode_step_rows as _decode_rows drives it: 40 rows over the 3 windows, each window's rows starting at a call of its
    own, two rows that are never active between them"""
    dec, xa, z, _, _ = S.decoder("s", dev)
    alone, want = solo("s", dev)
    names = step_names(dec, 40)
    R.check_small_en_step_families(40, names)
    tokens = torch.from_numpy(z["tokens"]).to(dev)
    T = tokens.shape[1]
    rows, first_call, idle = 40, {0: 0, 1: 1, 2: 3}, (7, 21)
    window = [WINDOW_OF_ROW[r % len(WINDOW_OF_ROW)] for r in range(rows)]
    assert all(0 < r < rows - 1 for r in idle) and len({window[r] for r in range(rows) if r not in idle}) == 3
    kc = whisper.KVCache(dec, xa, torch.tensor(window, dtype=torch.int32), T, per_row=True)
    for t in kc.self_k + kc.self_v:
        t.fill_(CANARY)
    lib, desc = S._lib.load(), S.C.byref(dec._w()["desc"])
    seen = 0
    for call in range(T + max(first_call.values())):
        pos = [-1 if r in idle or not 0 <= call - first_call[window[r]] < T else call - first_call[window[r]] for r in range(rows)]
        ctl = whisper.new_row_ctl([(p, 0, T, 0, 0, 0.0) for p in pos], dev)
        ids = torch.tensor([int(z["tokens"][window[r], max(p, 0)]) for r, p in enumerate(pos)], dtype=torch.int32, device=dev)
        S._lib.check(lib.hirest_whisper_decode_step_rows(desc, rows, ctl.data_ptr(), ids.data_ptr(), kc.k_ptrs, kc.v_ptrs, kc.T_max, kc.x_ptrs,
                                                         kc.n_windows, kc.Tk, kc.row_window.data_ptr(), kc.logits.data_ptr(), kc.ws.data_ptr(),
                                                         kc.ws.numel(), S.ops.stream_ptr()), "hirest_whisper_decode_step_rows")
        logits = kc.logits[:, :dec.vocab]
        for r, p in enumerate(pos):
            if p >= 0:
                assert torch.equal(logits[r], alone[p][window[r]]), (call, r, p, float((logits[r] - alone[p][window[r]]).abs().max()))
                assert float((logits[r].double() - want[window[r], p]).abs().max()) <= 4 * float(z["err32"])
                seen += 1
    assert seen == (rows - len(idle)) * T
    for i in range(dec.layers):
        for r in idle:
            assert bool((kc.self_k[i][r] == CANARY).all()) and bool((kc.self_v[i][r] == CANARY).all()), (i, r)
        active = [r for r in range(rows) if r not in idle]
        assert not bool((kc.self_k[i][active] == CANARY).any()) and not bool((kc.self_v[i][active] == CANARY).any())


@pytest.mark.parametrize("case", ["w384", "w512", "w1024", "w1280"])
def test_checkpoint_widths(case, dev):
    dec, xa, z, want, _ = S.decoder(case, dev)
    tokens = torch.from_numpy(z["tokens"]).to(dev)
    T, yard = tokens.shape[1], float(z["err32"])
    fused = {"w512": "m16ln<2,1,2>", "w1024": "m16ln<4,1,2>"}.get(case)
    for rows in (3, 40):
        names = step_names(dec, rows)
        for call in ("qkv", "cross_q", "fc1", "head"):
            assert names[call + "_fused"] == (fused is not None) and names[call][0] == 0, (case, rows, names)
            if fused:
                assert names[call][1] == fused, (case, rows, names)
        # the ln entry refuses the widths ln_gemm sends through hirest_layernorm + hirest_gemm_f32
        q = S._lib.GemmF32Query.make("ln", rows, 3 * dec.width, dec.width)
        status = S._lib.load().hirest_gemm_f32_dispatch_name(S.C.byref(q), S.C.create_string_buffer(64), 64)
        assert (status == 0) == (fused is not None), (case, rows, status)
    got = dec(torch.from_numpy(z["tokens"]), xa).cpu().double().numpy()
    e_forced = float(np.abs(got - want).max())
    assert got.shape == want.shape and e_forced <= 4 * yard, (e_forced, yard)
    want_d = torch.from_numpy(want).to(dev)
    stepped, e_step = {}, 0.0
    for rows in (3, 40):
        kc = whisper.KVCache(dec, xa, torch.zeros(rows, dtype=torch.int32), T)
        out = []
        for t in range(T):
            logits = dec.step(tokens[0, t].expand(rows).contiguous(), kc)[:, :dec.vocab]
            assert bool((logits == logits[0]).all()), (case, rows, t)
            e_step = max(e_step, float((logits.double() - want_d[0, t]).abs().max()))
            out.append(logits[0].clone())
        stepped[rows] = torch.stack(out)
    print(f"decoder {case}: max |got - fp64| / fp32 CPU forward (bar 4): teacher-forced {e_forced / yard:.2f}, stepped {e_step / yard:.2f}; "
          f"kernels at 3 rows { {k: v[1] for k, v in step_names(dec, 3).items() if not k.endswith('_fused')} }")
    assert e_step <= 4 * yard
    diff = float((stepped[40] - stepped[3]).abs().max())
    assert torch.equal(stepped[40], stepped[3]), (case, "40 rows against 3 rows", diff)


def test_decode_and_decode_many_at_small_en_width(dev):
    if "s" not in S._MODELS:
        S._MODELS["s"] = S.model_for("s", dev)
    model = S._MODELS["s"]
    _, xa, z, _, _ = S.decoder("s", dev)
    want, (avg, nsp, err32, margin) = z["greedy_00_tokens"].tolist(), z["greedy_00_stats"]
    res = whisper.decode(model, xa[0], whisper.DecodingOptions(temperature=0.0))
    print(f"greedy s: {len(res.tokens)} tokens, avg_logprob {res.avg_logprob:.6f} (fp64 {avg:.6f}), no_speech {res.no_speech_prob:.3e} "
          f"(fp64 {nsp:.3e}), fixture's smallest margin {margin:.2e}")
    assert res.tokens == want
    assert abs(res.avg_logprob - avg) <= 4 * err32 and abs(res.no_speech_prob - nsp) <= 4 * err32
    assert res.temperature == 0.0 and res.text == model.tokenizer.decode(want).strip()
    windows = [xa[w % 3] for w in range(9)]
    opts = [whisper.DecodingOptions(temperature=0.4, best_of=5, seed=11 + w) for w in range(9)]
    # the references: the lock-step loop of each window alone, 5 rows (R <= 32: the other kernel family than the 45 rows below)
    single = [lockstep_decode(model, w, o) for w, o in zip(windows, opts)]
    assert all(len(c) == 5 for c, _ in single) and len({tuple(t) for c, _ in single for t, _ in c}) > 9
    many, cands = whisper.decode_many(model, windows, opts, return_candidates=True)
    assert len(many) == len(cands) == 9
    for w in range(9):
        assert cands[w] == single[w][0] and many[w].no_speech_prob == single[w][1], (w, cands[w], single[w])
        t, lp = max(single[w][0], key=lambda c: c[1] / max(len(c[0]), 1))        # the pick among the reference's candidates (first on ties)
        assert (many[w].tokens, many[w].avg_logprob, many[w].temperature) == (t, lp / (len(t) + 1), 0.4), (w, many[w].tokens, t)
        assert many[w].text == model.tokenizer.decode(t).strip()
    for w in (0, 4):                                                  # decode(): the same loop with one window's 5 rows
        res, res_c = whisper.decode(model, windows[w], opts[w], return_candidates=True)
        assert same_result(res, many[w]) and res_c == single[w][0] and res.no_speech_prob == single[w][1], w
