"""The Whisper audio encoder at precision "bf16x3" (csrc/whisper_enc_x3.hip, AudioEncoder.set_precision) on the device.

Yardstick: tests/_whisper_enc_ref.py, the fp64 restatement of the encoder with every Linear product and both attention products formed
from the bf16 hi + lo splits of their operands — the format's own error and nothing else (its unsplit form is pinned to the goldens by
tests/test_whisper_x3_host.py).  The device may differ from the exact result by 4 x what that split run differs by: the project's
margin for summation order.  Nothing here widens with what the device gives; every figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest
import torch

import _whisper_enc_ref as R
from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENC_SEED = 73                          # make_whisper_golden.py's


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


_CASES = {}


def case(name, dev):
    """(config, state dict, mel, golden fp64 output, fp32 yard, x3 yard, fp32 encoder, bf16x3 encoder) — built once, never modified"""
    if name not in _CASES:
        cfg, clips = synth.WHISPER_CASES[name]
        sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
        mel = synth.whisper_mel_input(cfg, clips, ENC_SEED)
        z = np.load(os.path.join(GOLDEN, f"whisper_enc_{name}.npz"))
        want = torch.from_numpy(z["out"]).double()
        x3_yard = float((R.encoder(cfg, sd, mel, split=True) - want).abs().max())
        _CASES[name] = (cfg, sd, mel, want, float(z["yard"]), x3_yard, whisper.AudioEncoder(cfg, sd).to(dev),
                        whisper.AudioEncoder(cfg, sd).to(dev).set_precision("bf16x3"))
    return _CASES[name]


def against_restatement(cfg, sd, mel, got, what):
    """max |got - fp64| <= 4 x max |split restatement - fp64|, both against the unsplit restatement computed here"""
    want = R.encoder(cfg, sd, mel)
    yard = float((R.encoder(cfg, sd, mel, split=True) - want).abs().max())
    err = float((got.cpu().double() - want).abs().max())
    print(f"{what}: max |x3 - fp64| {err:.3e}, x3 yard {yard:.3e}, ratio {err / yard:.2f} (bar 4), max |ref| {float(want.abs().max()):.2f}")
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert err <= 4 * yard


# ------------------------------------------------------------------------------------------------------------- 1. accuracy
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_encoder_x3_against_golden(name, dev):
    cfg, sd, mel, want, yard32, yard, enc32, enc = case(name, dev)
    got = enc(mel.to(dev))
    assert got.dtype == torch.float32 and got.shape == want.shape and got.device.type == "cuda"
    err = float((got.cpu().double() - want).abs().max())
    f32 = enc32(mel.to(dev))
    err32 = float((f32.cpu().double() - want).abs().max())
    print(f"encoder x3 {name}: max |x3 - golden| {err:.3e}, x3 yard {yard:.3e}, ratio {err / yard:.2f} (bar 4); fp32 path {err32:.3e}, fp32 yard "
          f"{yard32:.3e}: x3 error = {err / yard32:.1f} x the fp32 yard; max |ref| {float(want.abs().max()):.2f}")
    assert err <= 4 * yard
    assert not torch.equal(got, f32)                                                      # the split kernels ran, not the fp32 path
    assert torch.equal(got, enc.embed_audio(mel.to(dev)))                                 # and the same bits on every run


# ------------------------------------------------------------------------------------------------------------- 2. released widths
@pytest.mark.parametrize("width,heads", [(384, 6), (512, 8), (768, 12), (1024, 16), (1280, 20)])
def test_released_widths(width, heads, dev):
    cfg = {"num_mel_bins": 80, "d_model": width, "encoder_attention_heads": heads, "encoder_layers": 1, "encoder_ffn_dim": 4 * width,
           "max_source_positions": 70}
    sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED + width)
    mel = synth.whisper_mel_input(cfg, 2, ENC_SEED + width)
    enc = whisper.AudioEncoder(cfg, sd).to(dev).set_precision("bf16x3")
    against_restatement(cfg, sd, mel, enc(mel.to(dev)), f"encoder x3 width {width} / {heads} heads")


# ------------------------------------------------------------------------------------------------------------- 3. production length
def test_production_length(dev):
    """ctx 1500 = 46 full waves of queries and one of 28, the long-sequence launch geometry of the split-operand attention"""
    cfg = synth.WHISPER_E2E
    sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
    mel = synth.whisper_mel_input(cfg, 1, ENC_SEED)
    enc = whisper.AudioEncoder(cfg, sd).to(dev).set_precision("bf16x3")
    against_restatement(cfg, sd, mel, enc(mel.to(dev)), "encoder x3 ctx 1500")


@pytest.mark.parametrize("B,T,H,dh", [(1, 1500, 2, 64), (2, 1500, 3, 32), (4, 1500, 11, 32)])
def test_attention_x3_at_1500_keys(B, T, H, dh, dev):
    """hirest_attention_x3_qkv alone at the encoder's length against fp64 (test_attention_x3_against_fp64's inputs and bar), and the
    automatic geometry bit-equal to the 4-wave and the 8-wave one: the workgroup size changes who stages the keys, not a query's
    arithmetic.  The automatic choice at 47 waves of queries is eight-wave workgroups once B x H x 6 of them fill the 256 CUs (the
    third case: 264), four-wave ones below (the first two)."""
    lib = _lib.load()
    D = H * dh
    qkv = synth.tensor(f"x3.attn.{B}.{T}.{H}.{dh}", (B * T, 3 * D), 1.0, 13).to(dev)
    qkv[:, :D] *= 3.0
    scale = dh ** -0.5
    q, k, v = (qkv[:, i * D:(i + 1) * D].double().reshape(B, T, H, dh).permute(0, 2, 1, 3) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * T, D)

    def run():
        out = torch.full((B * T, D), 7.0, dtype=torch.float32, device=dev)
        _lib.check(lib.hirest_attention_x3_qkv(qkv.data_ptr(), 3 * D, qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, out.data_ptr(), B, T, T,
                                               H, dh, scale, ops.stream_ptr()), "hirest_attention_x3_qkv")
        return out
    out = run()
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"attention x3 B={B} T={T} H={H} dh={dh}: max err / max |ref| {err:.2e} (bar 3e-5)")
    assert bool(torch.isfinite(out).all()) and err < 3e-5
    out2 = torch.empty((B * T, 2 * D), dtype=torch.bfloat16, device=dev)
    _lib.check(lib.hirest_attention_x3_qkv_split2(qkv.data_ptr(), 3 * D, qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, out2.data_ptr(), B, T, T,
                                                  H, dh, scale, ops.stream_ptr()), "hirest_attention_x3_qkv_split2")
    assert torch.equal(out2.view(torch.int16), ops.split2(out).view(torch.int16))
    for waves in (4, 8):
        _lib.check(lib.hirest_attention_x3_select_waves(waves), "select_waves")
        try:
            forced = run()
        finally:
            lib.hirest_attention_x3_select_waves(0)
        assert torch.equal(out, forced), waves


# ------------------------------------------------------------------------------------------------------------- 4. independence of rows
def test_clips_do_not_depend_on_the_batch(dev):
    cfg, sd, mel, _, _, _, _, enc = case("a", dev)
    mel = mel.to(dev)
    batched = enc(mel)
    for b in range(mel.shape[0]):
        assert torch.equal(enc(mel[b:b + 1])[0], batched[b]), b
        assert torch.equal(enc(mel[b])[0], batched[b]), b


def test_other_stream_same_bits(dev):
    """the scratch of the C call is per stream (ops.stream_workspace): a call on a side stream neither shares it nor differs"""
    cfg, sd, mel, _, _, _, _, enc = case("b", dev)
    mel = mel.to(dev)
    want = enc(mel)
    torch.cuda.synchronize()
    before = {k for k in ops._STREAM_WS if k[2] == "whisper_encoder_x3"}
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = enc(mel)
    side.synchronize()
    after = {k for k in ops._STREAM_WS if k[2] == "whisper_encoder_x3"}
    assert torch.equal(got, want) and len(after) == len(before) + 1


# ------------------------------------------------------------------------------------------------------------- 5. nothing else moved
def test_precisions_side_by_side(dev):
    cfg, clips = synth.WHISPER_CASES["a"]
    sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
    mel = synth.whisper_mel_input(cfg, clips, ENC_SEED).to(dev)
    enc = whisper.AudioEncoder(cfg, sd).to(dev)
    calls = {"fp32": 0, "x3": 0}
    f32_prepare, x3_prepare = enc.prepared_weights, enc.prepared_weights_x3

    def counted(kind, fn):
        def wrapper():
            calls[kind] += 1
            return fn()
        return wrapper
    enc.prepared_weights, enc.prepared_weights_x3 = counted("fp32", f32_prepare), counted("x3", x3_prepare)
    assert enc.precision == "fp32"
    before, stem = enc(mel), enc(mel, return_stem=True)
    assert calls == {"fp32": 1, "x3": 0}
    enc.set_precision("bf16x3")
    assert calls == {"fp32": 1, "x3": 0}                                                   # setting prepares nothing
    x3 = enc(mel)
    assert torch.equal(enc(mel, return_stem=True), stem)                                   # the stem is exact fp32 in both
    assert torch.equal(x3, case("a", dev)[7](mel)) and not torch.equal(x3, before)
    enc.set_precision("fp32")
    assert torch.equal(enc(mel), before) and torch.equal(enc(mel, return_stem=True), stem)
    enc.set_precision("bf16x3")
    assert torch.equal(enc(mel), x3)
    assert calls == {"fp32": 1, "x3": 1}                                                   # both stay resident: nothing is prepared twice
    assert enc._cache is not None and set(enc._cache_kinds) == {"x3"}
    # 4 bytes per Linear parameter beside the fp32 masters: bf16 hi + lo
    split = sum(t[n].numel() * t[n].element_size() for t in enc._cache_kinds["x3"]["keep"] for n in ("qkv_w2", "out_w2", "fc1_w2", "fc2_w2"))
    D, F = cfg["d_model"], cfg["encoder_ffn_dim"]
    assert split == 4 * cfg["encoder_layers"] * (4 * D * D + 2 * D * F)
    enc.float()                                                                            # a cast drops every kind together
    assert enc._cache is None and enc._cache_kinds == {}
    assert torch.equal(enc(mel), x3) and calls == {"fp32": 2, "x3": 2}


# ------------------------------------------------------------------------------------------------------------- 6. through the model
MODEL_MEL_SEED, MODEL_DEC_SEED, MODEL_EOT_BIAS = 73, 83, 0.5      # the committed seed of test_through_the_model (chosen on an MI355X)


def through_the_model(dev, mel_seed, dec_seed, eot_bias):
    """The figures of test_through_the_model for one seed: (fp32 tokens, x3 tokens, ended by eot, smallest top-2 margin of the teacher-forced
    fp32 logits along the fp32 greedy path, largest |logit difference| between the precisions on that path) and the x3 model + mel"""
    cfg = {**synth.WHISPER_DEC_P, **synth.WHISPER_E2E}
    eot = 100
    sd = {**{"encoder." + k: v for k, v in synth.whisper_encoder_state_dict(cfg, ENC_SEED).items()},
          **synth.whisper_decoder_state_dict(cfg, dec_seed, eot, eot_bias)}
    tok = synth.whisper_tokenizer(eot)
    m32, mx3 = whisper.Whisper(cfg, sd, tok).to(dev), whisper.Whisper(cfg, sd, tok).to(dev).set_precision("bf16x3")
    mel = synth.whisper_mel_input(cfg, 1, mel_seed).to(dev)
    opts = whisper.DecodingOptions(temperature=0.0, without_timestamps=True)
    r32, rx3 = m32.decode(mel[0], opts), mx3.decode(mel[0], opts)
    initial, _ = whisper._initial_tokens(tok, opts, m32.dims["n_text_ctx"])
    seq = (list(initial) + list(r32.tokens))[:m32.dims["n_text_ctx"]]
    first = len(initial) - 1                                       # the row that predicts the first sampled token; the last row predicts eot
    tokens = torch.tensor([seq], dtype=torch.int64, device=dev)
    l32 = m32.logits(tokens, m32.embed_audio(mel))[0, first:, :cfg["vocab_size"]].double()
    lx3 = mx3.logits(tokens, mx3.embed_audio(mel))[0, first:, :cfg["vocab_size"]].double()
    top2 = l32.topk(2, dim=-1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    diff = float((l32 - lx3).abs().max())
    return r32, rx3, margin, diff, mx3, mel


def test_through_the_model(dev):
    """A synthetic Whisper (the ctx-1500 encoder config with WHISPER_DEC_P's decoder) whose encoder runs at bf16x3.  The decoder is untouched:
    decode() of a window equals decode() of the states the x3 encoder gave it, bit for bit.  Greedy tokens equal the fp32 model's on the
    committed seed, whose fp32 greedy path is long enough and decided by margins far above what the precision moves a logit by — both
    checked here, and FAILED on, not skipped.
    Measured on an MI355X for the committed seed (decoder seed 83, mel seed 73): a greedy path of 24 tokens (the sample limit; two
    distinct ids), smallest top-2 margin 2.934e-2, largest |logit difference| 5.72e-6: margin / difference 5128, against the 4 needed.
    (Of the 12 seeds tried, every one gave equal tokens; the others' paths were one repeated id or shorter than 8.)"""
    r32, rx3, margin, diff, model, mel = through_the_model(dev, MODEL_MEL_SEED, MODEL_DEC_SEED, MODEL_EOT_BIAS)
    print(f"through the model: fp32 path {len(r32.tokens)} tokens, smallest top-2 margin {margin:.3e}, largest |logit difference| {diff:.3e} "
          f"(margin / difference {margin / max(diff, 1e-300):.1f}, needs > 4)")
    states = model.encoder(mel)
    assert model.precision == "bf16x3" and torch.equal(model.embed_audio(mel), states)
    opts = whisper.DecodingOptions(temperature=0.0, without_timestamps=True)
    given = model.decode(states[0], opts)
    assert (given.tokens, given.avg_logprob, given.no_speech_prob, given.text) == (rx3.tokens, rx3.avg_logprob, rx3.no_speech_prob, rx3.text)
    assert len(r32.tokens) >= 8                                                            # the seed's condition, part 1
    assert diff > 0.0 and margin > 4 * diff                                                # part 2
    assert rx3.tokens == r32.tokens
