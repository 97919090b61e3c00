"""The Whisper audio path on the device (hirest_amd/whisper.py, csrc/audio.hip) against the fixtures of
tests/golden/make_whisper_golden.py: the log-mel front end against the fp64 restatement of whisper/audio.py, hirest_mel_to_rows, the
convolution stem against fp64 conv1d, the encoder against transformers' WhisperEncoder in fp64, batch / schema invariance and
encode_file end to end.  Inputs and weights are rebuilt from hirest_amd.synth; nothing here needs transformers.

Measured on an MI355X (printed by the tests; the bars are the fixtures' own yardsticks, not these numbers):
    log-mel  max |got - fp64| / yard (yard = the error of Whisper's own fp32 arithmetic; bar 1):
             tone + noise 0.035, noise 0.138, click 0.187, 30 s mixed window 0.003, silence exactly -1.5
    stem     max |got - fp64| 1.3e-7 (a) / 1.6e-7 (b) against bars of 2.4e-7 / 2.6e-7
    encoder  max |got - fp64| / yard (yard = the fp32 CPU forward's error; bar 4):  a 1.05, b 0.75, c 0.76

"""
import os
import wave

import numpy as np
import pytest
import torch

from hirest_amd import _lib, ops, synth, whisper

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AUDIO_SEED, ENC_SEED = 71, 73          # make_whisper_golden.py's


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def mel_golden():
    return dict(np.load(os.path.join(GOLDEN, "whisper_mel.npz")))


_ENCODERS = {}


def encoder(case, dev):
    """(AudioEncoder on the device, its synth state dict, the case's input, fp64 output, yard): built once per case, never modified"""
    if case not in _ENCODERS:
        cfg, clips = synth.WHISPER_CASES[case]
        sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
        z = np.load(os.path.join(GOLDEN, f"whisper_enc_{case}.npz"))
        _ENCODERS[case] = (whisper.AudioEncoder(cfg, sd).to(dev), sd, synth.whisper_mel_input(cfg, clips, ENC_SEED),
                           torch.from_numpy(z["out"]), float(z["yard"]))
    return _ENCODERS[case]


# ---------------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("case", list(synth.AUDIO_CASES))
def test_log_mel_against_fp64(case, dev, mel_golden):
    """At least as close to the exact spectrogram as whisper/audio.py's own fp32 arithmetic is (yard); silence is exactly -1.5."""
    kind, n, padding = synth.AUDIO_CASES[case]
    got = whisper.log_mel_spectrogram(synth.audio_clip(kind, n, AUDIO_SEED), padding=padding, device=dev)
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (80, (n + padding) // 160) and got.is_contiguous()
    want, yard = torch.from_numpy(mel_golden[f"{case}_mel"]), float(mel_golden[f"{case}_yard"])
    got = got.cpu()[:, torch.from_numpy(mel_golden[f"{case}_frames"])]
    err = float((got.double() - want.double()).abs().max())
    print(f"log-mel {case}: max |got - fp64| {err:.3e}, yard {yard:.3e}, ratio {err / yard if yard else 0.0:.3f}")
    if case == "silence":
        assert yard == 0.0 and bool((got == -1.5).all())
    assert err <= yard


def test_log_mel_128_bins_and_tensor_input(dev, mel_golden):
    """The 128-row bank (large-v3's): against the 80-row result through the banks' own relation is not available, so the fp64 formula is
    restated here on the device-independent parts — power spectrum by torch.fft in double — for a short clip."""
    audio = synth.audio_clip("tone_noise", 2000, AUDIO_SEED)
    got = whisper.log_mel_spectrogram(torch.from_numpy(audio).to(dev), n_mels=128)
    assert got.shape == (128, 12) and got.device == dev
    a = torch.from_numpy(audio).double()
    stft = torch.stft(a, 400, 160, window=torch.hann_window(400, dtype=torch.float64), return_complex=True)
    mel = torch.from_numpy(whisper.mel_filters(128).copy()).double() @ (stft[..., :-1].abs() ** 2)
    log = torch.clamp(mel, min=1e-10).log10()
    want = (torch.maximum(log, log.max() - 8.0) + 4.0) / 4.0
    err = float((got.cpu().double() - want).abs().max())
    print(f"log-mel 128 bins: max |got - fp64| {err:.3e}")
    # two fp32 roundings (the log, |log| < 16: 2^-21 / 4; the result, < 2: 2^-24) bound the device's distance from the exact value
    assert err <= 2.0 ** -23 + 2.0 ** -24


def test_log_mel_invariances(dev):
    audio = synth.audio_clip("mixed", 40000, AUDIO_SEED + 1)
    a = whisper.log_mel_spectrogram(audio, padding=4321, device=dev)
    b = whisper.log_mel_spectrogram(np.concatenate([audio, np.zeros(4321, np.float32)]), device=dev)
    assert a.shape == b.shape == (80, 44321 // 160) and torch.equal(a, b)
    assert torch.equal(a, whisper.log_mel_spectrogram(audio, padding=4321, device=dev))
    with pytest.raises(ValueError):
        whisper.log_mel_spectrogram(np.zeros(200, np.float32), device=dev)
    assert whisper.log_mel_spectrogram(np.zeros(201, np.float32), device=dev).shape == (80, 1)


def test_log_mel_clamp_is_over_the_whole_call(dev):
    """A loud second half lifts the floor of the quiet first half: the maximum is one reduction over every block of frames."""
    quiet, loud = synth.audio_clip("noise", 16000, 3) * 1e-4, synth.audio_clip("tone_noise", 16000, 4)
    alone = whisper.log_mel_spectrogram(quiet, device=dev)
    both = whisper.log_mel_spectrogram(np.concatenate([quiet, loud]), device=dev)
    floor = float(both.max()) - 2.0
    assert float(both.min()) >= floor - 1e-6 and float(alone[:, :90].min()) < floor - 0.1
    assert bool((both[:, :90] >= alone[:, :90]).all()) and bool((both[:, :90] > alone[:, :90]).any())


@pytest.mark.parametrize("B,n_mels,T", [(3, 80, 66), (1, 128, 194), (2, 80, 3000)])
def test_mel_to_rows(B, n_mels, T, dev):
    mel = synth.tensor("rows.mel", (B, n_mels, T), 1.0, 9).to(dev)
    rows = torch.full((B, T + 2, n_mels), float("nan"), device=dev)
    _lib.check(_lib.load().hirest_mel_to_rows(mel.data_ptr(), rows.data_ptr(), B, n_mels, T, ops.stream_ptr()), "hirest_mel_to_rows")
    want = torch.nn.functional.pad(mel.transpose(1, 2), (0, 0, 1, 1))
    assert torch.equal(rows, want)


# ---------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("case", ["a", "b"])
def test_stem_against_fp64_conv1d(case, dev):
    """Two fp32 k-ordered chains (K = 240, then 3 d) and an erf each: 8 x 2^-24 x max |ref|.  The first and last row of every clip are
    where a wrong pad row would show."""
    enc, sd, mel, _, _ = encoder(case, dev)
    got = enc(mel.to(dev), return_stem=True).cpu().double()
    F = torch.nn.functional
    x = F.gelu(F.conv1d(mel.double(), sd["conv1.weight"].double(), sd["conv1.bias"].double(), padding=1))
    x = F.gelu(F.conv1d(x, sd["conv2.weight"].double(), sd["conv2.bias"].double(), stride=2, padding=1))
    want = x.permute(0, 2, 1) + sd["embed_positions.weight"].double()
    assert got.shape == want.shape == (mel.shape[0], enc.ctx, enc.width)
    bar = 8 * 2.0 ** -24 * float(want.abs().max())
    err = (got - want).abs()
    edge = float(torch.maximum(err[:, 0].max(), err[:, -1].max()))
    print(f"stem {case}: max |got - fp64| {float(err.max()):.3e} (first / last rows {edge:.3e}), bar {bar:.3e}, max |ref| {float(want.abs().max()):.3f}")
    assert edge <= bar
    assert float(err.max()) <= bar


# ---------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_encoder_against_fp64(case, dev):
    """max |got - fp64| <= 4 x the error of the same module's fp32 CPU forward: our GEMMs sum K in order where the CPU BLAS sums in
    blocks, so two fp32 evaluations differ by a small multiple of each other's error.  The ratio is printed."""
    enc, _, mel, want, yard = encoder(case, dev)
    got = enc(mel.to(dev))
    assert got.dtype == torch.float32 and got.shape == want.shape and got.device.type == "cuda"
    err = float((got.cpu().double() - want.double()).abs().max())
    print(f"encoder {case}: max |got - fp64| {err:.3e}, yard {yard:.3e}, ratio {err / yard:.2f} (bar 4)")
    assert err <= 4 * yard
    assert torch.equal(got, enc.embed_audio(mel.to(dev)))
    if case == "c":
        assert _lib.load().hirest_gemm_f32_workspace_bytes(enc.ctx, enc.width, 3 * enc.width) > 0       # conv2 takes the split form here
    with pytest.raises(ValueError):
        enc(mel[:, :, :-2].to(dev))
    with pytest.raises(ValueError):
        enc(mel[:, :-1].to(dev))


def test_encoder_batch_and_schema_invariance(dev):
    enc, sd, mel, _, _ = encoder("a", dev)
    mel = mel.to(dev)
    batched = enc(mel)
    stem = enc(mel, return_stem=True)
    for b in range(mel.shape[0]):
        assert torch.equal(enc(mel[b:b + 1])[0], batched[b]), b
        assert torch.equal(enc(mel[b])[0], batched[b]), b                                  # [n_mels, 2 ctx] is one clip
        assert torch.equal(enc(mel[b], return_stem=True)[0], stem[b]), b
    cfg, _ = synth.WHISPER_CASES["a"]
    openai = {"encoder." + k: v for k, v in whisper._canonical(sd).items()}
    dims = {"n_mels": cfg["num_mel_bins"], "n_audio_ctx": cfg["max_source_positions"], "n_audio_state": cfg["d_model"],
            "n_audio_head": cfg["encoder_attention_heads"], "n_audio_layer": cfg["encoder_layers"]}
    assert "encoder.blocks.0.attn.query.weight" in openai and "encoder.ln_post.bias" in openai
    other = whisper.AudioEncoder(dims, openai).to(dev)
    assert torch.equal(other(mel), batched)


def test_encode_file_end_to_end(dev, tmp_path):
    """A 31 s wav -> two fixed 3000-frame windows of the file's one spectrogram (padding = 480000)."""
    cfg = synth.WHISPER_E2E
    enc = whisper.AudioEncoder(cfg, synth.whisper_encoder_state_dict(cfg, ENC_SEED)).to(dev)
    audio = synth.audio_clip("mixed", 31 * 16000, AUDIO_SEED)
    path = str(tmp_path / "clip.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.round(audio * 32767.0).astype("<i2").tobytes())
    out = whisper.encode_file(path, enc)
    assert out.shape == (2, 1500, 128) and out.dtype == torch.float32
    mel = whisper.log_mel_spectrogram(path, padding=480000, device=dev)
    assert mel.shape == (80, 6100)
    assert torch.equal(out[0], enc(mel[:, :3000])[0])
    assert torch.equal(out[1], enc(mel[:, 3000:6000])[0])
    assert bool(torch.isfinite(out).all()) and abs(float(out.pow(2).mean().sqrt()) - 1.0) < 0.2       # ln_post's output
