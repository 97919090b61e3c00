#!/usr/bin/env python3
"""Throughput of the Whisper audio path at small.en's shape (768 wide, 12 heads, 12 layers, 1500 tokens; synthetic weights): 30 s
windows per second through ``log_mel_spectrogram`` + ``AudioEncoder.forward`` for 1 and 8 windows per call, the split between the
front end, the convolution stem and the blocks (each timed on its own, a device synchronise closing every timed window), and the
encoder's rate as a fraction of the 157-TFLOP/s fp32 MFMA peak DESIGN.md uses for the joint model.  Operations are counted from the
shapes.  Each figure is the median with the min .. max spread over the repeats.  The decode leg: W windows through one
run of the decoding loop (``decode_many``) against W one-window runs of the same loop (W sequential ``decode`` calls) at small.en's
decoder shape; ``--prompt-len N`` gives every window N previous tokens as its prompt (``transcribe()`` with
``condition_on_previous_text`` carries up to 223), so that the prefill has a prompt to run; ``--graph`` adds, per
window count and per ``--graph-chunks`` value, ``decode_many(graph=True)`` against the eager ``decode_many``, the two
alternating call by call in the same process.  The detect leg: ``detect_language`` of W windows at multilingual small's decoder shape and the pieces of
that call; the step leg: the one ``hirest_whisper_decode_step_rows`` call inside it, alone.  The align leg:
``hirest_whisper_alignment_matrix`` and ``hirest_dtw_f32`` for one window at small.en's shape (12 layers, 72 selected heads, 1500 keys)
with 50 and 220 tokens, each timed on its own, beside the numpy restatement of both on the CPU (tests/_whisper_align_ref.py, fp32).

``--precision fp32 bf16x3`` times the encoder leg at each named precision (``AudioEncoder.set_precision``), alternating per
batch size; the FLOP count is the same, the fraction is of the 157-TFLOP/s fp32 peak for fp32 and of bf16 peak / 3 for bf16x3.
``--x3-ab`` adds the bf16x3 encoder's A/B runs: GELU + split as a separate pass, the GEMMs' own tile choice, 4-wave attention workgroups.

    python tools/whisper_bench.py [--repeats 7] [--warmup 2] [--batches 1 8] [--legs encoder decode detect step align]
                                  [--precision fp32] [--x3-ab]
                                  [--windows 1 2 4 8 16] [--prompt-len 0] [--graph] [--graph-chunks 8]
                                  [--detect_windows 1 16] [--align_tokens 50 220]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hirest_amd import synth, whisper  # noqa: E402

FP32_MFMA_PEAK = 157e12
BF16_MFMA_PEAK = 2500e12                # dense bf16; a bf16x3 product is three bf16 MFMAs, so its yardstick is a third of this
PEAKS = {"fp32": (FP32_MFMA_PEAK, "the fp32 MFMA peak"), "bf16x3": (BF16_MFMA_PEAK / 3, "bf16 MFMA peak / 3")}


def spread(xs, scale=1e3, unit="ms"):
    return f"{statistics.median(xs) * scale:.3f} {unit} ({min(xs) * scale:.3f} .. {max(xs) * scale:.3f})"


def encoder_flop(c):
    """(stem, blocks) multiply-adds x 2 of one window, from the shapes"""
    D, F, L, H, ctx, M = (c[k] for k in ("d_model", "encoder_ffn_dim", "encoder_layers", "encoder_attention_heads", "max_source_positions",
                                         "num_mel_bins"))
    stem = 2 * (2 * ctx) * (3 * M) * D + 2 * ctx * (3 * D) * D
    block = 2 * ctx * D * 3 * D + 2 * 2 * ctx * ctx * D + 2 * ctx * D * D + 2 * 2 * ctx * D * F
    return stem, L * block


def timed(fn, repeats, warmup, min_window=0.25):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    inner = max(1, int(min_window / max(time.perf_counter() - t0, 1e-6)))      # enough calls per window to time the kernels, not the clock
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner)
    return out


def x3_ab(enc, mel, a):
    """The bf16x3 encoder as shipped against each of its measurement switches (same arithmetic, other launches): GELU + split as a
    separate pass over an fp32 hidden activation, hirest_gemm_bf16's own tile choice (gemm_pp256x3 for the large products), and the
    attention with 4-wave workgroups instead of 8-wave ones.  Medians in ms; the shipped form is timed first and last."""
    from hirest_amd import _lib
    lib = _lib.load()
    enc.set_precision("bf16x3")
    enc(mel)
    desc = enc._cache_kinds["x3"]["desc"]
    out = {}

    def run(name, flags=0, waves=0):
        desc.flags = flags
        lib.hirest_attention_x3_select_waves(waves)
        try:
            ts = timed(lambda: enc(mel), a.repeats, a.warmup)
        finally:
            desc.flags = 0
            lib.hirest_attention_x3_select_waves(0)
        out[name] = [round(x * 1e3, 4) for x in ts]
        print(f"        x3 A/B B = {mel.shape[0]} {name:28s} {spread(ts)}")
    run("shipped")
    run("gelu_separate_pass", _lib.WHISPER_X3_GELU_PASS)
    run("gemm_auto_tiles", _lib.WHISPER_X3_AUTO_TILES)
    run("gemm_auto_tiles+gelu_pass", _lib.WHISPER_X3_AUTO_TILES | _lib.WHISPER_X3_GELU_PASS)
    run("attention_4_waves", 0, 4)
    run("attention_3_waves", 0, 3)
    run("shipped_again")
    # the per-kernel split of the shipped form from the library's per-launch event records (one call)
    lib.hirest_profile_enable(1)
    enc(mel)
    torch.cuda.synchronize()
    recs = (_lib.ProfRecord * 4096)()
    n = lib.hirest_profile_collect(recs, len(recs))
    lib.hirest_profile_enable(0)
    groups = {}
    for r in recs[:max(n, 0)]:
        g = groups.setdefault((r.kind, r.tag, r.d0, r.d1, r.d2), [0, 0.0])
        g[0] += 1
        g[1] += r.ms
    kernels = []
    for (kind, tag, d0, d1, d2), (count, ms) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        kernels.append({"kind": {0: "gemm", 1: "attention", 2: "rows"}.get(kind, kind), "tag": tag, "dims": [d0, d1, d2], "launches": count,
                        "ms_per_call": round(ms, 5), "ms_per_launch": round(ms / count, 5)})
        print(f"        x3 kernels B = {mel.shape[0]} {kernels[-1]}")
    out["kernels"] = kernels
    return out


def decode_leg(a, dev):
    """W windows of small.en's shape (random weights, random encoder states) with best_of 5 and 64 forced steps — the eot embedding is
    biased so far down that no row ends — through one decode_many() loop against W sequential decode() calls, which are W one-window
    runs of the same loop, in the same process; and the same two with one step, which is the prefill and everything else a window
    costs before its loop: that call's time is the "prefill ms" column.  ``--prompt-len N``: every window's prompt is <|startofprev|>,
    N seeded text tokens (cut to the 223 the context admits) and <|startoftranscript|>; 0: <|startoftranscript|> alone.
    ``--graph``: after a window count's row, the same decode_many() with ``graph=True`` at every ``--graph-chunks`` length against the
    eager call — eager and replayed calls alternate, one of each per repeat — with the spread of both."""
    cfg = synth._dec_config(768, 12, 12, 1500, 51864, 448)
    eot, steps = 50256, 64
    sd = synth.whisper_decoder_state_dict(cfg, 83, eot, -8.0)
    sd.update({"encoder." + k: v for k, v in synth.whisper_encoder_state_dict({**cfg, "encoder_layers": 1}, 73).items()})
    tok = synth.whisper_tokenizer(eot)
    tok.decode = lambda ids: ""                                       # random weights pick ids the synthetic vocabulary cannot spell; no text is needed
    model = whisper.Whisper({**cfg, "encoder_layers": 1}, sd, tok).to(dev)                                 # the encoder is not run: states go in
    prompt = synth.token_ids("bench.decode.prompt", a.prompt_len, eot, 11).tolist() if a.prompt_len > 0 else None
    full = whisper.DecodingOptions(temperature=0.4, best_of=5, seed=5, sample_len=steps, prompt=prompt)
    one = whisper.DecodingOptions(temperature=0.4, best_of=5, seed=5, sample_len=1, prompt=prompt)
    n_initial = len(whisper._initial_tokens(tok, full, cfg["max_target_positions"])[0])
    xa_all = synth.whisper_audio_states(cfg, max(a.windows), 7).to(dev)
    print(f"decode: small.en's decoder shape, best_of 5, {n_initial} initial tokens per window, {steps} forced steps, medians of {a.repeats} "
          f"after {a.warmup} warm-up calls")
    print("   W | decode_many: windows/s  ms/step  prefill ms  prefill share | W x decode (W one-window loops): windows/s  ms/step  prefill ms  "
          "prefill share | ratio")
    table = {}
    for W in a.windows:
        xa = xa_all[:W]
        res, cands = whisper.decode_many(model, xa, full, return_candidates=True)
        assert all(len(t) == steps for c in cands for t, _ in c), "a row ended before its forced steps: lower the eot bias"
        assert [r.tokens for r in res] == [whisper.decode(model, xa[w], full).tokens for w in range(W)]
        med = lambda fn: statistics.median(timed(fn, a.repeats, a.warmup, min_window=0.0))
        many, many1 = med(lambda: whisper.decode_many(model, xa, full)), med(lambda: whisper.decode_many(model, xa, one))
        seq = med(lambda: [whisper.decode(model, xa[w], full) for w in range(W)])
        seq1 = med(lambda: [whisper.decode(model, xa[w], one) for w in range(W)])
        row = {"initial_tokens": n_initial, "many_windows_per_s": W / many, "many_ms_per_step": (many - many1) / (steps - 1) * 1e3,
               "many_prefill_ms": many1 * 1e3, "many_prefill_share": many1 / many,
               "sequential_windows_per_s": W / seq, "sequential_ms_per_step": (seq - seq1) / (steps - 1) / W * 1e3,
               "sequential_prefill_ms": seq1 * 1e3, "sequential_prefill_share": seq1 / seq}
        table[str(W)] = row
        print(f"  {W:2d} | {row['many_windows_per_s']:22.2f}  {row['many_ms_per_step']:7.3f}  {row['many_prefill_ms']:10.3f}  "
              f"{row['many_prefill_share']:13.3f} | {row['sequential_windows_per_s']:21.2f}  {row['sequential_ms_per_step']:7.3f}  "
              f"{row['sequential_prefill_ms']:10.3f}  {row['sequential_prefill_share']:13.3f} | {seq / many:5.2f}")
        if a.graph:
            row["graph"] = {str(chunk): graph_rows(a, model, xa, full, one, steps, chunk, [r.tokens for r in res]) for chunk in a.graph_chunks}
    return table


def graph_rows(a, model, xa, full, one, steps, chunk, want_tokens):
    """decode_many eager and with graph=True at one chunk length, alternating call by call: windows/s, ms per step and the prefill share
    of each, medians with min .. max"""
    W = int(xa.shape[0])
    whisper.DECODE_GRAPH_CHUNK = chunk
    before = model.graph_stats()
    assert [r.tokens for r in whisper.decode_many(model, xa, full, graph=True)] == want_tokens, "the replayed loop differs from the eager one"
    replays = model.graph_stats()["replays"] - before["replays"]

    def once(options, graph):
        t0 = time.perf_counter()
        whisper.decode_many(model, xa, options, graph=graph)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t = {(g, k): [] for g in (False, True) for k in ("full", "one")}
    for i in range(a.warmup + a.repeats):
        for g in (False, True):
            for k, options in (("full", full), ("one", one)):
                dt = once(options, g)
                if i >= a.warmup:
                    t[(g, k)].append(dt)
    med = statistics.median
    out = {"replays_per_call": replays}
    for g, name in ((False, "eager"), (True, "graph")):
        f, o = t[(g, "full")], t[(g, "one")]
        out[name] = {"windows_per_s": W / med(f), "windows_per_s_min": W / max(f), "windows_per_s_max": W / min(f),
                     "ms_per_step": (med(f) - med(o)) / (steps - 1) * 1e3, "prefill_ms": med(o) * 1e3, "prefill_share": med(o) / med(f),
                     "call_ms": [round(x * 1e3, 4) for x in f]}
        r = out[name]
        print(f"     | W {W:2d} chunk {chunk:2d} {name}: windows/s {r['windows_per_s']:8.2f} ({r['windows_per_s_min']:.2f} .. {r['windows_per_s_max']:.2f})  "
              f"ms/step {r['ms_per_step']:.3f}  prefill ms {r['prefill_ms']:.3f}  prefill share {r['prefill_share']:.3f}"
              + (f"  replays per call {replays}" if g else ""))
    out["graph_over_eager"] = out["graph"]["windows_per_s"] / out["eager"]["windows_per_s"]
    print(f"     | W {W:2d} chunk {chunk:2d} graph / eager windows/s {out['graph_over_eager']:.3f}")
    return out


def step_rows_setup(model, xa, sot):
    """what one ``hirest_whisper_decode_step_rows`` call of <|startoftranscript|> at position 0 needs, row w against window w: the work
    inside ``detect_language`` (``TextDecoder.step_rows``), set up outside the timed call."""
    dec, dev, R = model.decoder, model.device, int(xa.shape[0])
    kc = whisper.KVCache(dec, xa, torch.arange(R, dtype=torch.int32), 1, per_row=True)
    ctl = whisper.new_row_ctl([(0, 0, 1, 0, 0, 0.0)] * R, dev)
    ids = torch.full((R,), sot, dtype=torch.int32, device=dev)
    return (lambda: dec.step_rows(ctl, ids, kc)), (kc, ctl, ids)


def small_decoder_model(dev, languages):
    """multilingual small's decoder shape (768 wide, 12 heads, 12 layers, 1500 audio positions, 51865 tokens) with random weights
    behind a one-layer encoder that is not run; ``languages`` language tokens in the slots after <|startoftranscript|>"""
    cfg = synth._dec_config(768, 12, 12, 1500, 51865, 448)
    eot = 50256
    sd = synth.whisper_decoder_state_dict(cfg, 83, eot, 0.0)
    sd.update({"encoder." + k: v for k, v in synth.whisper_encoder_state_dict({**cfg, "encoder_layers": 1}, 73).items()})
    sp = synth.whisper_special_tokens(eot)
    if languages:
        sp.update({f"<|{code}|>": eot + 2 + i for i, code in enumerate(list(whisper.LANGUAGES)[:languages])})
    tok = whisper.Tokenizer(*synth.whisper_vocab(eot), sp, language="en" if languages else None, task="transcribe" if languages else None)
    return whisper.Whisper({**cfg, "encoder_layers": 1}, sd, tok).to(dev), cfg


def detect_leg(a, dev):
    """``detect_language`` of W windows' encoder states at multilingual small's decoder shape, 99 languages, per call and per window;
    beside it the pieces of the same call, each timed on its own with a device synchronise closing every timed window: the cross key /
    value projection of the W windows (``TextDecoder.cross_kv``: 12 GEMMs of [W * 1500, 768] x [768, 1536]), ONE
    ``hirest_whisper_decode_step_rows`` call at R = W — the decoder pass itself — and ``hirest_whisper_language_tail``.  What is left
    of the call after the three is the host: the cache and workspace allocations, the records' upload and the read-back."""
    from hirest_amd import _lib, ops
    model, cfg = small_decoder_model(dev, 99)
    tok, lib = model.tokenizer, _lib.load()
    xa_all = synth.whisper_audio_states(cfg, max(a.detect_windows), 7).to(dev)
    print(f"detect: multilingual small's decoder shape, 99 languages, medians of {a.repeats} after {a.warmup} warm-up calls (min .. max)")
    table = {}
    for W in a.detect_windows:
        xa = xa_all[:W]
        tokens, probs = whisper.detect_language(model, xa)
        assert tokens.shape == (W,) and all(abs(sum(p.values()) - 1.0) < 1e-5 for p in probs)
        whole = timed(lambda: whisper.detect_language(model, xa), a.repeats, a.warmup)
        cross = timed(lambda: model.decoder.cross_kv(xa), a.repeats, a.warmup)
        step, keep = step_rows_setup(model, xa, tok.sot)
        step_t = timed(step, a.repeats, a.warmup)
        logits, L = keep[0].logits, len(tok.all_language_tokens)
        ids = torch.tensor(tok.all_language_tokens, dtype=torch.int32, device=dev)
        out_t, out_p = torch.empty(W, dtype=torch.int32, device=dev), torch.empty((W, L), dtype=torch.float32, device=dev)
        tail = timed(lambda: _lib.check(lib.hirest_whisper_language_tail(logits.data_ptr(), model.decoder.vocab_padded, W, model.decoder.vocab,
                                                                         ids.data_ptr(), L, out_t.data_ptr(), out_p.data_ptr(), ops.stream_ptr()),
                                        "hirest_whisper_language_tail"), a.repeats, a.warmup)
        med = statistics.median
        rest = med(whole) - med(cross) - med(step_t) - med(tail)
        print(f"  W = {W:2d}: detect_language {spread(whole)} = {med(whole) / W * 1e3:.3f} ms per window")
        print(f"          cross_kv {spread(cross)}, decode_step_rows at R = W {spread(step_t)}, language_tail {spread(tail, 1e6, 'us')}, "
              f"the rest (host) {rest * 1e3:.3f} ms")
        table[str(W)] = {"detect_ms": [round(x * 1e3, 4) for x in whole], "detect_ms_per_window": med(whole) / W * 1e3,
                         "cross_kv_ms": [round(x * 1e3, 4) for x in cross], "step_rows_ms": [round(x * 1e3, 4) for x in step_t],
                         "language_tail_us": [round(x * 1e6, 3) for x in tail], "rest_ms": rest * 1e3}
    return table


def step_leg(a, dev):
    """one ``hirest_whisper_decode_step_rows`` call at R = W alone (``step_rows_setup``)"""
    model, cfg = small_decoder_model(dev, 0)
    xa_all = synth.whisper_audio_states(cfg, max(a.detect_windows), 7).to(dev)
    table = {}
    for W in a.detect_windows:
        step, keep = step_rows_setup(model, xa_all[:W], model.tokenizer.sot)
        t = timed(step, a.repeats, a.warmup)
        print(f"step: hirest_whisper_decode_step_rows at R = W = {W:2d}, position 0, T_max 1: {spread(t)}")
        table[str(W)] = {"step_rows_ms": [round(x * 1e3, 4) for x in t]}
    return table


def align_leg(a, dev):
    """One window's alignment at small.en's shape: the cross-attention queries of T tokens in 12 layers, the heads of the last 6 layers
    (72 pairs), 1500 keys, filter width 7 -> the [T - 2, 1500] matrix (``hirest_whisper_alignment_matrix``, five kernels in 9
    launches) and the path through its negative (``hirest_dtw_f32`` with the read-back of the path, as ``dtw`` returns it); inputs
    are seeded at unit scale and stay resident.  The CPU column is the numpy restatement of the same two steps in fp32, once."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import numpy as np
    import _whisper_align_ref as A
    L, H, Tk, D = 12, 12, 1500, 768
    pairs = [(l, h) for l in range(L // 2, L) for h in range(H)]
    kv = [synth.tensor(f"bench.align.kv.{l}", (Tk, 2 * D), 1.0, 7) for l in range(L)]
    kv_dev = [t.to(dev) for t in kv]
    print(f"align: small.en's shape, {len(pairs)} heads, {Tk} keys, medians of {a.repeats} after {a.warmup} warm-up calls (min .. max)")
    table = {}
    for T in a.align_tokens:
        q = [synth.tensor(f"bench.align.q.{l}", (T, D), 1.0, 8) for l in range(L)]
        q_dev = [t.to(dev) for t in q]
        ws = torch.empty((len(pairs) * T * Tk * 4,), dtype=torch.uint8, device=dev)
        run = lambda: whisper.alignment_matrix(q_dev, kv_dev, pairs, Tk, heads=H, row0=1, n_rows=T - 2, workspace=ws)
        matrix = run()
        t_matrix = timed(run, a.repeats, a.warmup)
        t_dtw = timed(lambda: whisper.dtw_many([matrix], negate=True), a.repeats, a.warmup)
        t0 = time.perf_counter()
        ref = A.alignment_matrix([t.numpy() for t in q], [t.numpy() for t in kv], pairs, Tk, row0=1, n_rows=T - 2, dtype=np.float32)
        t1 = time.perf_counter()
        ti, tj = A.dtw(-matrix.cpu().numpy(), dtype=np.float32)
        t2 = time.perf_counter()
        gi, gj = whisper.dtw_many([matrix], negate=True)[0]
        assert gi.tolist() == ti.tolist() and gj.tolist() == tj.tolist() and float(np.abs(ref - matrix.cpu().numpy()).max()) < 1e-4
        print(f"  T = {T:3d}: alignment matrix {spread(t_matrix)}, dtw [{T - 2}, {Tk}] with its read-back {spread(t_dtw)}; "
              f"numpy on the CPU: matrix {(t1 - t0) * 1e3:.0f} ms, dtw {(t2 - t1) * 1e3:.0f} ms")
        table[str(T)] = {"matrix_ms": [round(x * 1e3, 4) for x in t_matrix], "dtw_ms": [round(x * 1e3, 4) for x in t_dtw],
                         "numpy_matrix_ms": (t1 - t0) * 1e3, "numpy_dtw_ms": (t2 - t1) * 1e3}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--precision", nargs="+", choices=list(whisper.AudioEncoder.PRECISIONS), default=["fp32"],
                    help="encoder leg: the precisions to time, in this order for every batch size")
    ap.add_argument("--x3-ab", action="store_true", help="encoder leg: also the bf16x3 encoder under each of its measurement switches")
    ap.add_argument("--legs", nargs="+", choices=["encoder", "decode", "detect", "step", "align"], default=["encoder", "decode"])
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 2, 4, 8, 16], help="windows per decode_many() call of the decode leg")
    ap.add_argument("--prompt-len", type=int, default=0, help="previous tokens in every window's prompt of the decode leg (0: none, as before)")
    ap.add_argument("--graph", action="store_true", help="decode leg: also decode_many(graph=True), alternating with the eager call")
    ap.add_argument("--graph-chunks", type=int, nargs="+", default=[whisper.DECODE_GRAPH_CHUNK],
                    help="decode leg with --graph: iterations per captured graph (whisper.DECODE_GRAPH_CHUNK) to time")
    ap.add_argument("--detect_windows", type=int, nargs="+", default=[1, 16], help="windows per detect_language() call of the detect leg")
    ap.add_argument("--align_tokens", type=int, nargs="+", default=[50, 220], help="tokens of the teacher-forced pass of the align leg")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("whisper_bench needs an MI355X: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    if "encoder" not in a.legs:
        legs = {"decode": decode_leg, "detect": detect_leg, "step": step_leg, "align": align_leg}
        print(json.dumps({"device": torch.cuda.get_device_name(0), **{leg: legs[leg](a, dev) for leg in a.legs}}))
        return
    cfg = synth.WHISPER_SMALL_EN
    enc = whisper.AudioEncoder(cfg, synth.whisper_encoder_state_dict(cfg, 73)).to(dev)
    audio = torch.from_numpy(synth.audio_clip("mixed", whisper.N_SAMPLES, 71)).to(dev)
    stem_flop, block_flop = encoder_flop(cfg)
    front = timed(lambda: whisper.log_mel_spectrogram(audio), a.repeats, a.warmup)
    print(f"{torch.cuda.get_device_name(0)}, small.en's encoder shape, {a.repeats} repeats after {a.warmup} warm-up calls")
    print(f"front end, one 30 s window (resident waveform -> [80, 3000])   {spread(front)}")
    result = {"device": torch.cuda.get_device_name(0), "front_end_ms": [round(x * 1e3, 4) for x in front], "batches": {}}
    mel1 = whisper.log_mel_spectrogram(audio)
    for B in a.batches:
        mel = mel1[None].expand(B, -1, -1).contiguous()
        for precision in a.precision:
            enc.set_precision(precision)
            peak, peak_name = PEAKS[precision]
            stem = timed(lambda: enc(mel, return_stem=True), a.repeats, a.warmup)
            whole = timed(lambda: enc(mel), a.repeats, a.warmup)
            t_front, t_stem, t_whole = (statistics.median(x) for x in (front, stem, whole))
            t_blocks = t_whole - t_stem
            per_window = t_front + t_whole / B
            print(f"B = {B} {precision}: encoder {spread(whole)}, of which stem {spread(stem)} ({t_stem / t_whole:.3f} of it)")
            print(f"        windows/s {1.0 / per_window:.1f} with one front-end call per window; shares: front end {t_front / per_window:.3f}, "
                  f"stem {t_stem / B / per_window:.3f}, blocks {t_blocks / B / per_window:.3f}")
            print(f"        encoder {B * (stem_flop + block_flop) / t_whole / 1e12:.1f} TFLOP/s = {B * (stem_flop + block_flop) / t_whole / peak:.3f} of "
                  f"{peak_name} (stem {B * stem_flop / t_stem / 1e12:.1f}, blocks {B * block_flop / t_blocks / 1e12:.1f} TFLOP/s = "
                  f"{B * block_flop / t_blocks / peak:.3f}); a whole-call rate, launches and row operations included")
            entry = {"encoder_ms": [round(x * 1e3, 4) for x in whole], "stem_ms": [round(x * 1e3, 4) for x in stem],
                     "windows_per_s": 1.0 / per_window, "front_end_share": t_front / per_window,
                     "encoder_tflops": B * (stem_flop + block_flop) / t_whole / 1e12}
            if precision == "fp32":                                    # (the keys this tool has always printed)
                entry["fraction_of_fp32_mfma_peak"] = B * (stem_flop + block_flop) / t_whole / peak
                result["batches"][str(B)] = entry
            else:
                entry["fraction_of_bf16_mfma_peak_over_3"] = B * (stem_flop + block_flop) / t_whole / peak
                result.setdefault("batches_" + precision, {})[str(B)] = entry
        if a.x3_ab:
            result.setdefault("x3_ab", {})[str(B)] = x3_ab(enc, mel, a)
    enc.set_precision("fp32")
    for leg, fn in (("decode", decode_leg), ("detect", detect_leg), ("step", step_leg), ("align", align_leg)):
        if leg in a.legs:
            result[leg] = fn(a, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
