#!/usr/bin/env python
"""Fixtures of the Whisper audio path: tests/golden/whisper_mel.npz and whisper_enc_{a,b,c}.npz.

Whisper is not part of the reference tree, so the yardsticks come from ``transformers`` (WhisperFeatureExtractor, WhisperEncoder) and
from an fp64 restatement of ``whisper/audio.py::log_mel_spectrogram`` on ``torch.stft``.  Inputs and weights are ``hirest_amd.synth``'s,
rebuilt from their seeds by the tests; the GPU tests read only these files.

    python tests/golden/make_whisper_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hirest_amd import synth  # noqa: E402

AUDIO_SEED, ENC_SEED = 71, 73


def log_mel(audio: np.ndarray, padding: int, filters: np.ndarray, dtype) -> torch.Tensor:
    """whisper/audio.py::log_mel_spectrogram, statement for statement, in ``dtype`` (fp32 is what Whisper itself runs)."""
    a = torch.nn.functional.pad(torch.from_numpy(audio).to(dtype), (0, padding))
    window = torch.hann_window(400, dtype=dtype)
    stft = torch.stft(a, 400, 160, window=window, return_complex=True)
    magnitudes = stft[..., :-1].abs() ** 2
    mel_spec = torch.from_numpy(filters).to(dtype) @ magnitudes
    log_spec = torch.clamp(mel_spec, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def mixed_frames(frames: int) -> np.ndarray:
    return np.array(list(range(16)) + list(range(16, frames - 16, 7)) + list(range(frames - 16, frames)), dtype=np.int64)


def gen_mel():
    from transformers import WhisperFeatureExtractor
    from transformers.audio_utils import mel_filter_bank
    banks = {n: mel_filter_bank(num_frequency_bins=201, num_mel_filters=n, min_frequency=0.0, max_frequency=8000.0, sampling_rate=16000,
                                norm="slaney", mel_scale="slaney").T.copy() for n in (80, 128)}
    fe = WhisperFeatureExtractor()
    assert np.array_equal(fe.mel_filters.T, banks[80])
    out = {"filters_80": banks[80], "filters_128": banks[128]}
    f32 = banks[80].astype(np.float32)                      # Whisper's asset is fp32
    for case, (kind, n, padding) in synth.AUDIO_CASES.items():
        audio = synth.audio_clip(kind, n, AUDIO_SEED)
        exact = log_mel(audio, padding, f32, torch.float64)
        single = log_mel(audio, padding, f32, torch.float32)
        assert exact.shape == (80, (n + padding) // 160)
        lib = fe._np_extract_fbank_features(np.pad(audio, (0, padding))[None], "cpu")[0]
        d_lib = float(np.abs(lib - exact.numpy()).max())
        assert d_lib <= 5e-5, (case, d_lib)
        keep = mixed_frames(exact.shape[1]) if case == "mixed" else np.arange(exact.shape[1])
        yard = float((single.double() - exact)[:, keep].abs().max())
        on_clamp = float((exact == exact.min()).double().mean())
        print(f"mel {case}: frames {exact.shape[1]} (kept {keep.size}), yard {yard:.3e}, feature extractor vs fp64 {d_lib:.3e}, "
              f"range {float(exact.min()):.3f} .. {float(exact.max()):.3f}, at the minimum {on_clamp:.2f}")
        out[f"{case}_mel"] = exact[:, keep].float().numpy()
        out[f"{case}_frames"] = keep
        out[f"{case}_yard"] = np.float64(yard)
    assert np.all(out["silence_mel"] == -1.5) and out["silence_yard"] == 0.0
    np.savez_compressed(os.path.join(HERE, "whisper_mel.npz"), **out)


def gen_encoder():
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    for case, (cfg, clips) in synth.WHISPER_CASES.items():
        config = WhisperConfig(**cfg, decoder_layers=1, decoder_attention_heads=cfg["encoder_attention_heads"], decoder_ffn_dim=64,
                               activation_function="gelu", attn_implementation="eager")
        enc = WhisperEncoder(config).eval()
        sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
        enc.load_state_dict(sd, strict=True)
        mel = synth.whisper_mel_input(cfg, clips, ENC_SEED)
        with torch.no_grad():
            single = enc(mel).last_hidden_state.double()
            exact = enc.double()(mel.double()).last_hidden_state
        yard = float((single - exact).abs().max())
        print(f"encoder {case}: out {tuple(exact.shape)}, rms {float(exact.pow(2).mean().sqrt()):.3f}, yard {yard:.3e}")
        np.savez(os.path.join(HERE, f"whisper_enc_{case}.npz"), out=exact.float().numpy(), yard=np.float64(yard))


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_mel()
    gen_encoder()
    for f in sorted(os.listdir(HERE)):
        if f.startswith("whisper_"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 512 * 1024, (f, size)
            print(f, size)
