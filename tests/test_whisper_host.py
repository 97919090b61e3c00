"""Host side of the Whisper audio path (hirest_amd/whisper.py): the mel filter bank against the transformers banks of the fixture, the
frame-count rule, pad_or_trim, load_audio and its refusals, both checkpoint schemas, the MI355X-only errors, and the weight reorder
that turns the stem's convolutions into products over overlapping views of zero-padded channel-last rows."""
import os
import wave

import numpy as np
import pytest
import torch

from hirest_amd import synth, whisper

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def write_wav(path, samples, rate=16000, channels=1, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples).astype({1: np.uint8, 2: "<i2", 4: "<i4"}[width]).tobytes())


@pytest.mark.parametrize("n_mels", [80, 128])
def test_mel_filters_match_the_published_bank(n_mels):
    want = np.load(os.path.join(GOLDEN, "whisper_mel.npz"))[f"filters_{n_mels}"]
    got = whisper.mel_filters(n_mels)
    assert got.dtype == np.float32 and got.shape == (n_mels, 201) == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9)
    assert (got >= 0).all() and (got.sum(1) > 0).all()
    with pytest.raises(ValueError):
        whisper.mel_filters(64)


def test_frame_count_rule():
    assert whisper.N_SAMPLES == 480000 and whisper.N_FRAMES == 3000
    for n, p, want in ((1600, 0, 10), (1000, 0, 6), (480000, 0, 3000), (330000, 150000, 3000), (496000, 480000, 6100), (201, 0, 1), (319, 1, 2)):
        assert whisper.n_frames(n, p) == want
    for case, (_, n, p) in synth.AUDIO_CASES.items():
        z = np.load(os.path.join(GOLDEN, "whisper_mel.npz"))
        assert int(z[f"{case}_frames"].max()) + 1 == whisper.n_frames(n, p)


def test_pad_or_trim():
    a = np.arange(10, dtype=np.float32)
    assert np.array_equal(whisper.pad_or_trim(a, 4), a[:4])
    assert np.array_equal(whisper.pad_or_trim(a, 13), np.concatenate([a, np.zeros(3, np.float32)]))
    assert whisper.pad_or_trim(a, 10) is a or np.array_equal(whisper.pad_or_trim(a, 10), a)
    t = torch.arange(12.0).reshape(3, 4)
    assert torch.equal(whisper.pad_or_trim(t, 2), t[:, :2])
    assert torch.equal(whisper.pad_or_trim(t, 6), torch.cat([t, torch.zeros(3, 2)], 1))
    assert torch.equal(whisper.pad_or_trim(t, 5, axis=0), torch.cat([t, torch.zeros(2, 4)], 0))
    assert torch.equal(whisper.pad_or_trim(t, 2, axis=0), t[:2])
    assert whisper.pad_or_trim(np.zeros(7, np.float32)).shape == (480000,)
    assert np.array_equal(whisper.pad_or_trim(np.arange(12.0).reshape(3, 4), 6, axis=0)[3:], np.zeros((3, 4)))


def test_load_audio_and_its_refusals(tmp_path):
    pcm = (np.arange(-400, 400) * 80).astype(np.int16)
    write_wav(tmp_path / "ok.wav", pcm)
    got = whisper.load_audio(str(tmp_path / "ok.wav"))
    assert got.dtype == np.float32 and np.array_equal(got, pcm.astype(np.float32) / 32768.0)
    write_wav(tmp_path / "rate.wav", pcm, rate=44100)
    with pytest.raises(ValueError, match="44100"):
        whisper.load_audio(str(tmp_path / "rate.wav"))
    write_wav(tmp_path / "stereo.wav", np.repeat(pcm, 2), channels=2)
    with pytest.raises(ValueError, match="2 channels"):
        whisper.load_audio(str(tmp_path / "stereo.wav"))
    write_wav(tmp_path / "wide.wav", pcm.astype(np.int32), width=4)
    with pytest.raises(ValueError, match="4 bytes"):
        whisper.load_audio(str(tmp_path / "wide.wav"))


def openai_checkpoint(cfg, sd):
    """The same tensors as OpenAI's .pt holds them (dims + model_state_dict, encoder.* names, a decoder tensor beside them)."""
    names = {"embed_positions.weight": "positional_embedding", "layers.": "blocks.", "self_attn.q_proj": "attn.query",
             "self_attn.k_proj": "attn.key", "self_attn.v_proj": "attn.value", "self_attn.out_proj": "attn.out",
             "self_attn_layer_norm": "attn_ln", "final_layer_norm": "mlp_ln", "fc1": "mlp.0", "fc2": "mlp.2"}
    out = {}
    for k, v in sd.items():
        if k.startswith("layer_norm."):
            k = "ln_post." + k[len("layer_norm."):]
        else:
            for a, b in names.items():
                k = k.replace(a, b)
        out["encoder." + k] = v
    out["decoder.token_embedding.weight"] = torch.zeros(4, cfg["d_model"])
    dims = {"n_mels": cfg["num_mel_bins"], "n_audio_ctx": cfg["max_source_positions"], "n_audio_state": cfg["d_model"],
            "n_audio_head": cfg["encoder_attention_heads"], "n_audio_layer": cfg["encoder_layers"], "n_vocab": 4, "n_text_ctx": 4,
            "n_text_state": cfg["d_model"], "n_text_head": 1, "n_text_layer": 1}
    return {"dims": dims, "model_state_dict": out}


def hf_directory(path, cfg, sd, prefix="model.encoder."):
    import json
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(cfg, model_type="whisper", activation_function="gelu"), f)
    torch.save({prefix + k: v for k, v in sd.items()}, os.path.join(path, "pytorch_model.bin"))
    return str(path)


def test_both_checkpoint_schemas_prepare_the_same_weights(tmp_path):
    cfg = synth.WHISPER_TINY_B
    sd = synth.whisper_encoder_state_dict(cfg, 73)
    assert set(sd) == set(synth.whisper_encoder_shapes(cfg)) and not any("k_proj.bias" in k for k in sd)
    torch.save(openai_checkpoint(cfg, sd), tmp_path / "tiny.pt")
    a = whisper.load_encoder(str(tmp_path / "tiny.pt"))
    b = whisper.load_encoder(hf_directory(tmp_path / "hf", cfg, sd))
    c = whisper.AudioEncoder(cfg, {"encoder." + k: v for k, v in sd.items()})          # WhisperModel's own prefix, explicit config
    assert a.dims == b.dims == c.dims == {"n_mels": 80, "ctx": 97, "width": 128, "heads": 4, "layers": 2, "ffn": 512}
    pa, pb, pc = a.prepared_weights(), b.prepared_weights(), c.prepared_weights()
    assert set(pa) == set(pb) == set(pc)
    for k in pa:
        assert torch.equal(pa[k], pb[k]) and torch.equal(pa[k], pc[k]), k
    assert pa["qkv_w.0"].shape == (3 * 128, 128) and pa["conv1_w"].shape == (128, 240) and pa["conv2_w"].shape == (128, 384)
    assert torch.equal(pa["qkv_w.1"][128:256], sd["layers.1.self_attn.k_proj.weight"])
    assert not pa["qkv_b.0"][128:256].any() and pa["qkv_b.0"][:128].any()              # the key projection has no bias
    assert all(not p.requires_grad for p in a.parameters())
    a._cache = {"stale": None}
    a.float()
    assert a._cache is None                                                               # any move / cast drops the fused operands
    with pytest.raises(KeyError):
        whisper.AudioEncoder(cfg, {k: v for k, v in sd.items() if k != "conv2.bias"})


def test_narrow_heads_are_padded_with_zero_lanes():
    cfg = dict(synth.WHISPER_TINY_A, d_model=80, encoder_attention_heads=4, encoder_ffn_dim=160)     # 20-wide heads: 4 x 20 = 80
    enc = whisper.AudioEncoder(cfg, synth.whisper_encoder_state_dict(cfg, 5))
    assert (enc.dh, enc.ah) == (20, 20) and (enc.heads * enc.ah) % 16 == 0
    cfg = dict(synth.WHISPER_TINY_A, d_model=48, encoder_attention_heads=8, encoder_ffn_dim=96)      # 6-wide heads -> 8 lanes each
    enc = whisper.AudioEncoder(cfg, synth.whisper_encoder_state_dict(cfg, 5))
    assert (enc.dh, enc.ah) == (6, 8)
    p = enc.prepared_weights()
    assert p["qkv_w.0"].shape == (3 * 64, 48) and p["o_w.0"].shape == (48, 64)
    assert not p["qkv_w.0"].view(3, 8, 8, 48)[:, :, 6:].any() and not p["o_w.0"].view(48, 8, 8)[:, :, 6:].any()
    assert torch.equal(p["qkv_w.0"].view(3, 8, 8, 48)[1, :, :6].reshape(48, 48), enc._p("blocks.0.attn.key.weight"))


def test_hub_names_are_not_downloaded():
    for name in ("small.en", "openai/whisper-small.en"):
        with pytest.raises(FileNotFoundError):
            whisper.load_encoder(name)


def test_no_cpu_fallback():
    cfg = synth.WHISPER_TINY_A
    enc = whisper.AudioEncoder(cfg, synth.whisper_encoder_state_dict(cfg, 73))
    with pytest.raises(RuntimeError, match="MI355X only"):
        enc(synth.whisper_mel_input(cfg, 1, 73))
    with pytest.raises(RuntimeError, match="MI355X only"):
        enc.embed_audio(synth.whisper_mel_input(cfg, 1, 73))
    with pytest.raises(RuntimeError, match="MI355X only"):
        whisper.log_mel_spectrogram(np.zeros(1600, np.float32), device="cpu")
    with pytest.raises(ValueError, match="200"):                    # the reflect padding of the first frame is undefined
        whisper.log_mel_spectrogram(np.zeros(200, np.float32), device="cpu")
    with pytest.raises(ValueError):
        whisper.log_mel_spectrogram(np.zeros((2, 1600), np.float32), device="cpu")


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_weight_reorder_against_conv1d(stride):
    """The product the kernels run — A[m, :] = 3 C consecutive floats of the zero-padded channel-last rows, starting stride * C after
    row m - 1, times conv_as_gemm_weight(w)^T — is conv1d(k = 3, pad 1) at that stride."""
    g = torch.Generator().manual_seed(3 + stride)
    C, O, T = 12, 7, 26
    x = torch.randn((C, T), generator=g, dtype=torch.float64)
    w = torch.randn((O, C, 3), generator=g, dtype=torch.float64)
    want = torch.nn.functional.conv1d(x[None], w, stride=stride, padding=1)[0].T                 # [T / stride, O]
    rows = torch.zeros((T + 2, C), dtype=torch.float64)
    rows[1:T + 1] = x.T
    M = T // stride
    a = torch.as_strided(rows, (M, 3 * C), (stride * C, 1))
    assert (M - 1) * stride * C + 3 * C <= rows.numel()                                          # the view stays inside the padded rows
    got = a @ whisper.conv_as_gemm_weight(w).T
    assert got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
