"""Whisper's audio path on MI355X: the log-mel front end and the audio encoder, under Whisper's own names.

The reference transcribes every video's audio with ``whisper.load_model('small.en')`` (extraction/whisper_ASR/extract_ASR.py) before
the subtitles are embedded.  This module is the lower half of that stage, the part with the arithmetic (12 pre-LN layers over 1500
tokens, 0.34 TFLOP per 30 s window) and the part Whisper's users call directly::

    whisper.load_audio / pad_or_trim / log_mel_spectrogram        ->  the same names here
    model.embed_audio(mel) / model.encoder(mel)                   ->  AudioEncoder.embed_audio / AudioEncoder.forward

The text decoder, the tokenizer, ``transcribe()`` with its temperature fallback and ``.srt`` writing are not built.
Whisper is not under the reference tree; the front end restates ``whisper/audio.py`` and the encoder ``whisper/model.py::AudioEncoder``
from the published definitions, pinned against ``transformers``' WhisperFeatureExtractor / WhisperEncoder (tests/golden/whisper_*.npz).

MI355X side.  ``hirest_log_mel`` (csrc/audio.hip) accumulates the DFT and the mel sums in double and rounds to fp32 at the log, which puts
it closer to the exact spectrogram than the fp32 ``torch.stft`` Whisper itself runs.  The stem's two k = 3 convolutions are
``hirest_gemm_f32`` products over an overlapping view of channel-last rows with one zero row around each clip (``hirest_mel_to_rows``):
row m of the A operand starts ``stride * C`` floats after row m - 1 and is ``3 C`` long, so no im2col copy exists; the second one adds
the positional embedding in its epilogue, after the GELU.  The blocks run on the exact-fp32 kernels of the other encoders
(``hirest_gemm_f32`` / ``hirest_gemm_f32_ln`` / ``hirest_attention_f32`` / ``hirest_layernorm``).  There is no CPU path: ``forward`` and
``log_mel_spectrogram`` raise off-GPU.  A local ``.pt`` or model directory is required: nothing is downloaded.
"""
from __future__ import annotations

import functools
import json
import os
import wave
from typing import Dict, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .sentence_encoder import _AH_MAX, _load_weights

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE          # 480000 samples in a 30-second window
N_FRAMES = N_SAMPLES // HOP_LENGTH              # 3000 frames in a mel spectrogram input

_NAME = "hirest_amd.whisper"


def load_audio(path: str, sr: int = SAMPLE_RATE) -> np.ndarray:
    """A mono 16 kHz PCM16 ``.wav`` (what extract_audio.py writes with ffmpeg) -> float32 samples in [-1, 1).  Whisper pipes any file
    through ffmpeg; here anything but that one format raises ValueError naming what it found."""
    with wave.open(path, "rb") as w:
        if w.getnchannels() != 1:
            raise ValueError(f"{path}: {w.getnchannels()} channels (mono expected)")
        if w.getsampwidth() != 2:
            raise ValueError(f"{path}: sample width {w.getsampwidth()} bytes (16-bit PCM expected)")
        if w.getframerate() != sr:
            raise ValueError(f"{path}: sample rate {w.getframerate()} Hz ({sr} expected)")
        raw = w.readframes(w.getnframes())
    return np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0


def pad_or_trim(array, length: int = N_SAMPLES, *, axis: int = -1):
    """Pad with zeros or trim ``axis`` to ``length`` (numpy arrays and tensors, host or device)."""
    if torch.is_tensor(array):
        if array.shape[axis] > length:
            array = array.index_select(dim=axis, index=torch.arange(length, device=array.device))
        if array.shape[axis] < length:
            widths = [(0, 0)] * array.ndim
            widths[axis] = (0, length - array.shape[axis])
            array = torch.nn.functional.pad(array, [p for w in widths[::-1] for p in w])
        return array
    array = np.asarray(array)
    if array.shape[axis] > length:
        array = array.take(indices=range(length), axis=axis)
    if array.shape[axis] < length:
        widths = [(0, 0)] * array.ndim
        widths[axis] = (0, length - array.shape[axis])
        array = np.pad(array, widths)
    return array


@functools.lru_cache(maxsize=None)
def _mel_filters(n_mels: int) -> np.ndarray:
    def hz_to_mel(f):        # Slaney's scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)
        f = np.asarray(f, dtype=np.float64)
        return np.where(f < 1000.0, f * (3.0 / 200.0), 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * (27.0 / np.log(6.4)))

    def mel_to_hz(m):
        return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)))
    bins = np.linspace(0.0, SAMPLE_RATE / 2, N_FFT // 2 + 1)
    edges = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(SAMPLE_RATE / 2), n_mels + 2))
    up = (bins[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    down = (edges[2:, None] - bins[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    bank = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]      # triangles of unit area
    bank = bank.astype(np.float32)
    bank.setflags(write=False)
    return bank


def mel_filters(n_mels: int = 80) -> np.ndarray:
    """The ``[n_mels, 201]`` fp32 mel filter bank for 16 kHz audio and 400-point frames: Slaney's mel scale, triangles normalised to
    unit area (``librosa.filters.mel(sr=16000, n_fft=400, n_mels=n_mels)``, which Whisper ships as an asset; computed here)."""
    if n_mels not in (80, 128):
        raise ValueError(f"unsupported n_mels: {n_mels} (80 or 128)")
    return _mel_filters(int(n_mels))


def n_frames(n_samples: int, padding: int = 0) -> int:
    """Frames of ``log_mel_spectrogram``: the centred transform has 1 + (n + padding) // 160 frames and its last one is dropped."""
    return (int(n_samples) + int(padding)) // HOP_LENGTH


_DEVICE_TABLES = {}


def _tables(device: torch.device, n_mels: int):
    """(DFT twiddles + Hann window as 1200 doubles, filter bank) on ``device``, computed once in float64 on the host."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), n_mels)
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        ang = 2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT
        tab = np.concatenate([np.cos(ang), np.sin(ang), 0.5 - 0.5 * np.cos(ang)])
        hit = (torch.from_numpy(tab).to(device), torch.from_numpy(mel_filters(n_mels).copy()).to(device))
        _DEVICE_TABLES[key] = hit
    return hit


def _gpu_device(device, what: str) -> torch.device:
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type != "cuda":
        raise RuntimeError(f"{_NAME}.{what} runs on MI355X only (no CPU fallback); pass a GPU device")
    return dev


def log_mel_spectrogram(audio: Union[str, np.ndarray, torch.Tensor], n_mels: int = 80, padding: int = 0,
                        device: Optional[Union[str, torch.device]] = None) -> torch.Tensor:
    """``whisper.log_mel_spectrogram``: a path, numpy array or tensor of mono 16 kHz samples, with ``padding`` zeros appended ->
    ``[n_mels, (n + padding) // 160]`` fp32 on the device.  The clamp at "maximum - 8" uses the maximum of the whole call, as Whisper's
    does: the spectrogram of a file is one call, windows are cut from it afterwards."""
    if isinstance(audio, (str, os.PathLike)):
        audio = load_audio(os.fspath(audio))
    filters = mel_filters(n_mels)
    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    if audio.ndim != 1:
        raise ValueError(f"audio of shape {tuple(audio.shape)}: one mono waveform expected")
    n, padding = int(audio.numel()), int(padding)
    if padding < 0:
        raise ValueError(f"negative padding {padding}")
    if n <= N_FFT // 2:
        raise ValueError(f"audio of {n} samples: the reflect padding of the first frame needs more than {N_FFT // 2}")
    if device is None and audio.device.type == "cuda":
        device = audio.device
    dev = _gpu_device(device, "log_mel_spectrogram")
    with torch.cuda.device(dev):
        audio = audio.to(dev, torch.float32).contiguous()
        tab, bank = _tables(dev, filters.shape[0])
        lib = _lib.load()
        out = torch.empty((filters.shape[0], n_frames(n, padding)), dtype=torch.float32, device=dev)
        ws = torch.empty((lib.hirest_log_mel_workspace_bytes(n, padding),), dtype=torch.uint8, device=dev)
        _lib.check(lib.hirest_log_mel(audio.data_ptr(), n, padding, bank.data_ptr(), filters.shape[0], tab.data_ptr(), out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), ops.stream_ptr()), "hirest_log_mel")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------------------

def conv_as_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight ``[out, C, k]`` -> ``[out, k * C]`` with ``W[o, k C + c] = w[o, c, k]``: the operand of the product over channel-last
    rows, where the k taps of an output row are k consecutive rows of C channels."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def _dims(d) -> Dict[str, int]:
    """OpenAI ``ModelDimensions`` (object or dict: n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer) or a Hugging Face
    Whisper ``config.json`` dict -> the encoder's sizes."""
    get = (lambda k, default=None: d.get(k, default)) if isinstance(d, dict) else (lambda k, default=None: getattr(d, k, default))
    if get("n_audio_state") is not None:
        width = int(get("n_audio_state"))
        return {"n_mels": int(get("n_mels")), "ctx": int(get("n_audio_ctx")), "width": width, "heads": int(get("n_audio_head")),
                "layers": int(get("n_audio_layer")), "ffn": 4 * width}
    if get("d_model") is not None:
        if get("activation_function", "gelu") != "gelu":
            raise NotImplementedError(f"activation {get('activation_function')!r}: Whisper's erf GELU is what is built")
        width = int(get("d_model"))
        return {"n_mels": int(get("num_mel_bins")), "ctx": int(get("max_source_positions")), "width": width,
                "heads": int(get("encoder_attention_heads")), "layers": int(get("encoder_layers")),
                "ffn": int(get("encoder_ffn_dim", 4 * width))}
    raise ValueError("neither Whisper's ModelDimensions (n_audio_state ...) nor a Hugging Face Whisper config (d_model ...)")


_HF_TO_OPENAI = (("embed_positions.weight", "positional_embedding"), ("layers.", "blocks."), ("self_attn.q_proj", "attn.query"),
                 ("self_attn.k_proj", "attn.key"), ("self_attn.v_proj", "attn.value"), ("self_attn.out_proj", "attn.out"),
                 ("self_attn_layer_norm", "attn_ln"), ("final_layer_norm", "mlp_ln"), ("fc1", "mlp.0"), ("fc2", "mlp.2"))


def _canonical(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Either schema's encoder tensors under OpenAI's names without the ``encoder.`` prefix; decoder tensors are dropped."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith("model."):
            k = k[len("model."):]
        if k.startswith("decoder.") or k.startswith("proj_out."):
            continue
        if k.startswith("encoder."):
            k = k[len("encoder."):]
        if k.startswith("layers.") or k.startswith("embed_positions.") or k.startswith("layer_norm."):
            for a, b in _HF_TO_OPENAI:
                k = k.replace(a, b)
            if k.startswith("layer_norm."):
                k = "ln_post." + k[len("layer_norm."):]
        out[k] = v
    return out


class AudioEncoder(nn.Module):
    """``whisper.model.AudioEncoder``: conv1 (k 3) + GELU, conv2 (k 3, stride 2) + GELU, + positional embedding, pre-LN blocks, ln_post.

    ``dims_or_config``: OpenAI's ``ModelDimensions`` / ``dims`` dict or a Hugging Face ``config.json`` dict; ``state_dict`` in either
    schema (``encoder.blocks.i.attn.query ...`` or ``[model.]encoder.layers.i.self_attn.q_proj ...``; decoder tensors are ignored).
    The weights are frozen parameters under OpenAI's names; the fused operands are built on first use and dropped on any move / cast."""

    def __init__(self, dims_or_config, state_dict: Dict[str, torch.Tensor]):
        super().__init__()
        self.dims = _dims(dims_or_config)
        d = self.dims
        self.n_mels, self.ctx, self.width, self.heads, self.layers, self.ffn = (d[k] for k in ("n_mels", "ctx", "width", "heads", "layers", "ffn"))
        if self.width % self.heads or self.width % 16 or self.ffn % 16 or self.n_mels % 16:
            raise NotImplementedError(f"width {self.width} / heads {self.heads} / ffn {self.ffn} / n_mels {self.n_mels}: multiples of 16 expected")
        self.dh = self.width // self.heads
        if self.dh > _AH_MAX:
            raise NotImplementedError(f"head width {self.dh} > {_AH_MAX}")
        self.ah = (self.dh + 3) // 4 * 4               # head width as the kernels see it (zero lanes after dh) ...
        while (self.heads * self.ah) % 16:             # ... such that the output projection's reduction length suits the GEMM
            self.ah += 4
        self.eps = 1e-5
        sd = _canonical(state_dict)
        want = {"conv1.weight": (self.width, self.n_mels, 3), "conv1.bias": (self.width,), "conv2.weight": (self.width, self.width, 3),
                "conv2.bias": (self.width,), "positional_embedding": (self.ctx, self.width), "ln_post.weight": (self.width,),
                "ln_post.bias": (self.width,)}
        for i in range(self.layers):
            p = f"blocks.{i}."
            for n in ("query", "key", "value", "out"):
                want[p + f"attn.{n}.weight"] = (self.width, self.width)
                if n != "key":
                    want[p + f"attn.{n}.bias"] = (self.width,)
            want.update({p + "attn_ln.weight": (self.width,), p + "attn_ln.bias": (self.width,), p + "mlp_ln.weight": (self.width,),
                         p + "mlp_ln.bias": (self.width,), p + "mlp.0.weight": (self.ffn, self.width), p + "mlp.0.bias": (self.ffn,),
                         p + "mlp.2.weight": (self.width, self.ffn), p + "mlp.2.bias": (self.width,)})
        for k, shape in want.items():
            if k not in sd:
                raise KeyError(f"AudioEncoder: {k} missing from the state dict")
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"AudioEncoder: {k} has shape {tuple(sd[k].shape)}, expected {shape}")
            # parameter names cannot hold dots: keep the checkpoint's name with '/'
            self.register_parameter(k.replace(".", "/"), nn.Parameter(sd[k].detach().float().clone(), requires_grad=False))
        self._cache = None

    # nn.Module plumbing: any move / cast invalidates the fused-weight cache
    def _apply(self, fn, *a, **k):
        self._cache = None
        return super()._apply(fn, *a, **k)

    def _p(self, name: str) -> torch.Tensor:
        return self._parameters[name.replace(".", "/")]

    @property
    def device(self) -> torch.device:
        return self._p("conv1.weight").device

    def prepared_weights(self) -> Dict[str, torch.Tensor]:
        """The operands the kernels read, on the parameters' device: reordered convolution weights, per-block fused QKV (zero key bias,
        heads zero-padded to the attention kernel's width) and output projections."""
        f = lambda n: self._p(n).detach().float().contiguous()
        H, dh, AH, D = self.heads, self.dh, self.ah, self.width
        dev = self.device
        c = {"conv1_w": conv_as_gemm_weight(f("conv1.weight")), "conv1_b": f("conv1.bias"),
             "conv2_w": conv_as_gemm_weight(f("conv2.weight")), "conv2_b": f("conv2.bias"),
             "pos": f("positional_embedding"), "ln_post_w": f("ln_post.weight"), "ln_post_b": f("ln_post.bias")}

        def pad_rows(w, b):      # [H*dh, D] -> [H*AH, D]: head h's rows at AH h .. AH h + dh, zeros after (AH = dh: a copy)
            wp = torch.zeros((H, AH, D), device=dev); wp[:, :dh] = w.view(H, dh, D)
            bp = torch.zeros((H, AH), device=dev); bp[:, :dh] = b.view(H, dh)
            return wp.view(H * AH, D), bp.view(H * AH)
        for i in range(self.layers):
            p = f"blocks.{i}."
            ws, bs = zip(*(pad_rows(f(p + f"attn.{n}.weight"), f(p + f"attn.{n}.bias") if n != "key" else torch.zeros(D, device=dev))
                           for n in ("query", "key", "value")))
            c[f"qkv_w.{i}"] = torch.cat(ws, 0).contiguous()
            c[f"qkv_b.{i}"] = torch.cat(bs, 0).contiguous()
            wo = torch.zeros((D, H, AH), device=dev)
            wo[:, :, :dh] = f(p + "attn.out.weight").view(D, H, dh)
            c[f"o_w.{i}"] = wo.view(D, H * AH).contiguous()
            for n in ("attn.out.bias", "attn_ln.weight", "attn_ln.bias", "mlp_ln.weight", "mlp_ln.bias", "mlp.0.weight", "mlp.0.bias",
                      "mlp.2.weight", "mlp.2.bias"):
                c[p + n] = f(p + n)
        return c

    def _w(self):
        if self._cache is None:
            if self.device.type != "cuda":
                raise RuntimeError(f"{_NAME}.AudioEncoder runs on MI355X only (no CPU fallback); move the model to a GPU")
            self._cache = self.prepared_weights()
        return self._cache

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _gemm(a_ptr, lda, w, bias, out_ptr, ldo, M, device, act=0, resid=None, periodic=None, period=0):
        """out[M, N] = act(A W^T + bias) (+ resid) (+ periodic[m % period]) on raw operand addresses: A's rows may overlap"""
        lib = _lib.load()
        N, K = w.shape
        ws, wsb = ops.stream_workspace(device, lib.hirest_gemm_f32_workspace_bytes(M, N, K))
        _lib.check(lib.hirest_gemm_f32_ws(a_ptr, lda, w.data_ptr(), K, bias.data_ptr(), resid.data_ptr() if resid is not None else None, N,
                                          periodic.data_ptr() if periodic is not None else None, period, out_ptr, ldo, M, N, K, act,
                                          ws, wsb, ops.stream_ptr()), "hirest_gemm_f32_ws")

    def _linear(self, x, w, bias, act=0, resid=None):
        out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
        self._gemm(x.data_ptr(), x.shape[1], w, bias, out.data_ptr(), w.shape[0], x.shape[0], x.device, act=act, resid=resid)
        return out

    def _ln_linear(self, x, gamma, beta, w, bias, act=0):
        """act(LayerNorm(x) W^T + bias): inside one GEMM where hirest_gemm_f32_ln has a form for the shape (up to 256 rows, K a multiple
        of 256 up to 1024), else hirest_layernorm + hirest_gemm_f32 — the same bits either way."""
        M, K = x.shape
        N = w.shape[0]
        if M <= 256 and K % 256 == 0 and K <= 1024 and N < 8192:
            out = torch.empty((M, N), dtype=torch.float32, device=x.device)
            _lib.check(_lib.load().hirest_gemm_f32_ln(x.data_ptr(), K, None, None, None, gamma.data_ptr(), beta.data_ptr(), self.eps, None, 0,
                                                      w.data_ptr(), K, bias.data_ptr(), None, 0, out.data_ptr(), N, M, N, K, act,
                                                      ops.stream_ptr()), "hirest_gemm_f32_ln")
            return out
        return self._linear(ops.layernorm(x, gamma, beta, self.eps, torch.empty_like(x)), w, bias, act=act)

    def _stem(self, mel: torch.Tensor) -> torch.Tensor:
        """[B, n_mels, 2 ctx] -> [B * ctx, width]: gelu(conv2(gelu(conv1(mel)))) + positional embedding, per clip, as two products over
        overlapping views of zero-padded channel-last rows"""
        c, lib = self._w(), _lib.load()
        B, C, T = mel.shape
        D, ctx, dev = self.width, self.ctx, mel.device
        rows = torch.empty((B, T + 2, C), dtype=torch.float32, device=dev)
        _lib.check(lib.hirest_mel_to_rows(mel.data_ptr(), rows.data_ptr(), B, C, T, ops.stream_ptr()), "hirest_mel_to_rows")
        h = torch.empty((B, T + 2, D), dtype=torch.float32, device=dev)         # conv1's output, again with a zero row around each clip
        h[:, 0].zero_()
        h[:, T + 1].zero_()
        x = torch.empty((B * ctx, D), dtype=torch.float32, device=dev)
        for b in range(B):
            # conv1 (stride 1): output row t reads padded rows t, t + 1, t + 2 = 3 C consecutive floats from row t on
            self._gemm(rows[b].data_ptr(), C, c["conv1_w"], c["conv1_b"], h[b, 1].data_ptr(), D, T, dev, act=1)
            # conv2 (stride 2): output row t reads padded rows 2 t, 2 t + 1, 2 t + 2; GELU, then + positional embedding (row t of the clip)
            self._gemm(h[b].data_ptr(), 2 * D, c["conv2_w"], c["conv2_b"], x[b * ctx].data_ptr(), D, ctx, dev, act=1,
                       periodic=c["pos"], period=ctx)
        return x

    @torch.no_grad()
    def forward(self, mel: torch.Tensor, return_stem: bool = False) -> torch.Tensor:
        """``mel`` ``[B, n_mels, 2 ctx]`` or ``[n_mels, 2 ctx]`` -> ``[B, ctx, width]`` fp32 encoder states (``return_stem``: the input of
        the first block instead).  Any other frame count raises ValueError, where Whisper asserts."""
        if self.device.type != "cuda":
            raise RuntimeError(f"{_NAME}.AudioEncoder runs on MI355X only (no CPU fallback); move the model to a GPU")
        if mel.ndim == 2:
            mel = mel[None]
        if mel.ndim != 3 or mel.shape[1] != self.n_mels or mel.shape[2] != 2 * self.ctx:
            raise ValueError(f"mel of shape {tuple(mel.shape)}: [B, {self.n_mels}, {2 * self.ctx}] expected (incorrect audio shape)")
        dev = self.device
        with torch.cuda.device(dev):
            mel = mel.to(dev, torch.float32).contiguous()
            c, lib = self._w(), _lib.load()
            B, ctx, H, AH = mel.shape[0], self.ctx, self.heads, self.ah
            x = self._stem(mel)
            if return_stem:
                return x.view(B, ctx, self.width)
            for i in range(self.layers):
                p = f"blocks.{i}."
                qkv = self._ln_linear(x, c[p + "attn_ln.weight"], c[p + "attn_ln.bias"], c[f"qkv_w.{i}"], c[f"qkv_b.{i}"])
                att = torch.empty((B * ctx, H * AH), dtype=torch.float32, device=dev)
                _lib.check(lib.hirest_attention_f32(qkv.data_ptr(), att.data_ptr(), B, ctx, H, AH, self.dh ** -0.5, 0.0, ops.stream_ptr()),
                           "hirest_attention_f32")
                x = self._linear(att, c[f"o_w.{i}"], c[p + "attn.out.bias"], resid=x)
                hid = self._ln_linear(x, c[p + "mlp_ln.weight"], c[p + "mlp_ln.bias"], c[p + "mlp.0.weight"], c[p + "mlp.0.bias"], act=1)
                x = self._linear(hid, c[p + "mlp.2.weight"], c[p + "mlp.2.bias"], resid=x)
            out = ops.layernorm(x, c["ln_post_w"], c["ln_post_b"], self.eps, torch.empty_like(x))
        return out.view(B, ctx, self.width)

    embed_audio = forward


def load_encoder(path: str, device: Optional[Union[str, torch.device]] = None) -> AudioEncoder:
    """An OpenAI ``.pt`` checkpoint (a dict with ``dims`` and ``model_state_dict``) or a Hugging Face model directory (``config.json`` +
    ``model.safetensors`` / ``pytorch_model.bin``), picked by what ``path`` is.  A model name (``'small.en'``, ``'openai/whisper-small.en'``)
    raises FileNotFoundError: nothing is downloaded."""
    if os.path.isdir(path):
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        enc = AudioEncoder(config, _load_weights(path))
    elif os.path.isfile(path):
        ckpt = torch.load(path, map_location="cpu")
        if not (isinstance(ckpt, dict) and "dims" in ckpt and "model_state_dict" in ckpt):
            raise ValueError(f"{path}: not a Whisper checkpoint (a dict with 'dims' and 'model_state_dict')")
        enc = AudioEncoder(ckpt["dims"], ckpt["model_state_dict"])
    else:
        raise FileNotFoundError(f"{path!r} is neither a local .pt checkpoint nor a model directory (no network access: download the "
                                "model beforehand and pass its path)")
    return enc.to(device) if device is not None else enc


@torch.no_grad()
def encode_file(path: str, encoder: AudioEncoder) -> torch.Tensor:
    """Encoder states of a whole ``.wav``: ``[n_windows, ctx, width]``.  One spectrogram of the file with 30 s of zero padding
    (``padding = 480000``, as ``transcribe()`` computes it), cut into 3000-frame windows at a FIXED stride of 3000 frames, the last one
    zero-extended by that padding.  This is not ``transcribe()``'s walk: it seeks to the last decoded timestamp of each window, which
    needs the decoder; fixed windows are what the encoder can do on its own."""
    if 2 * encoder.ctx != N_FRAMES:
        raise ValueError(f"encode_file cuts {N_FRAMES}-frame windows: an encoder with n_audio_ctx {N_FRAMES // 2} is needed, not {encoder.ctx}")
    audio = load_audio(path)
    mel = log_mel_spectrogram(audio, encoder.n_mels, padding=N_SAMPLES, device=encoder.device)
    content = n_frames(audio.shape[0])                                # frames that hold audio; the rest is the padding
    n_windows = max(1, -(-content // N_FRAMES))
    windows = torch.stack([mel[:, w * N_FRAMES:(w + 1) * N_FRAMES] for w in range(n_windows)])
    return encoder(windows)
