"""Whisper on MI355X under Whisper's own names: the log-mel front end and the audio encoder, and (further down) the text
decoder, the tokenizer, ``decode()``, ``transcribe()`` and ``.srt`` writing.

The reference transcribes every video's audio with ``whisper.load_model('small.en')`` (extraction/whisper_ASR/extract_ASR.py) before
the subtitles are embedded.  This module is the lower half of that stage, the part with the arithmetic (12 pre-LN layers over 1500
tokens, 0.34 TFLOP per 30 s window) and the part Whisper's users call directly::

    whisper.load_audio / pad_or_trim / log_mel_spectrogram        ->  the same names here
    model.embed_audio(mel) / model.encoder(mel)                   ->  AudioEncoder.embed_audio / AudioEncoder.forward

    whisper.load_model / model.decode / whisper.transcribe / utils.write_srt  ->  the same names here (sampling branch; no beam search)
    whisper.detect_language / tokenizer.LANGUAGES / TO_LANGUAGE_CODE          ->  the same names here
    transcribe(word_timestamps=True) / whisper.timing.find_alignment, dtw ..  ->  the same names here

Whisper is not under the reference tree; the front end restates ``whisper/audio.py`` and the encoder ``whisper/model.py::AudioEncoder``
from the published definitions, pinned against ``transformers``' WhisperFeatureExtractor / WhisperEncoder (tests/golden/whisper_*.npz).

MI355X side.  ``hirest_log_mel`` (csrc/audio.hip) accumulates the DFT and the mel sums in double and rounds to fp32 at the log, which puts
it closer to the exact spectrogram than the fp32 ``torch.stft`` Whisper itself runs.  The stem's two k = 3 convolutions are
``hirest_gemm_f32`` products over an overlapping view of channel-last rows with one zero row around each clip (``hirest_mel_to_rows``):
row m of the A operand starts ``stride * C`` floats after row m - 1 and is ``3 C`` long, so no im2col copy exists; the second one adds
the positional embedding in its epilogue, after the GELU.  The blocks run on the exact-fp32 kernels of the other encoders
(``hirest_gemm_f32`` / ``hirest_gemm_f32_ln`` / ``hirest_attention_f32`` / ``hirest_layernorm``) or, after
``set_precision("bf16x3")``, on split bf16 operands in one C call (``hirest_whisper_encoder_x3_forward``).  There is no CPU path: ``forward`` and
``log_mel_spectrogram`` raise off-GPU.  A local ``.pt`` or model directory is required: nothing is downloaded.

What the two halves share is written once: the size and key tables of both checkpoint schemas (``_dims``, ``_canonical``, by side), the
checkpoint reader, the frozen-weights base of ``AudioEncoder`` and ``TextDecoder``, and ``_linear`` / ``_ln_linear``.  Decoding has ONE
token loop, ``_decode_rows`` over the per-row entry points: ``decode()`` runs it once per window, ``decode_many()`` once
for the windows of several files.  ``TextDecoder.forward(kv_cache=)`` / ``prefill`` / ``step`` over the lock-step ``KVCache`` stay as
Whisper's ``decoder(tokens, xa, kv_cache)`` surface; the lock-step loop over them is the tests' yardstick (tests/_whisper_lockstep.py).
"""
from __future__ import annotations

import collections
import copy
import ctypes as C
import dataclasses
import functools
import json
import os
import re
import string
import types
import wave
import zlib
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .bytebpe import ByteBPETokenizer
from .sentence_encoder import _AH_MAX, _fused_head_operands, _load_weights, _padded_head_width

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE          # 480000 samples in a 30-second window
N_FRAMES = N_SAMPLES // HOP_LENGTH              # 3000 frames in a mel spectrogram input

_NAME = "hirest_amd.whisper"
TOKENS_PER_SECOND = SAMPLE_RATE // HOP_LENGTH // 2      # 50 encoder positions (and timestamp tokens) per second
PREPEND_PUNCTUATIONS = "\"'“¿([{-"                       # whisper.transcribe's defaults
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
_TIMESTAMP = re.compile(r"<\|\d+\.\d\d\|>")


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


# Per side ("audio": the encoder, "text": the decoder): the name of the side's first size, OpenAI's ``ModelDimensions`` fields for
# (first size, ctx, width, heads, layers), and the Hugging Face ``config.json`` fields for the same five and the MLP width.
_DIM_FIELDS = {"audio": ("n_mels", ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer"),
                         ("num_mel_bins", "max_source_positions", "d_model", "encoder_attention_heads", "encoder_layers", "encoder_ffn_dim")),
               "text": ("vocab", ("n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer"),
                        ("vocab_size", "max_target_positions", "d_model", "decoder_attention_heads", "decoder_layers", "decoder_ffn_dim"))}


def _dims(d, side: str = "audio") -> Dict[str, int]:
    """OpenAI ``ModelDimensions`` (object or dict) or a Hugging Face Whisper ``config.json`` dict -> that side's sizes: ``n_mels``
    (audio) or ``vocab`` (text), ``ctx``, ``width``, ``heads``, ``layers``, ``ffn``."""
    first, openai, hf = _DIM_FIELDS[side]
    get = (lambda k, default=None: d.get(k, default)) if isinstance(d, dict) else (lambda k, default=None: getattr(d, k, default))
    if get(openai[2]) is not None:
        size, ctx, width, heads, layers = (int(get(k)) for k in openai)
        ffn = 4 * width
    elif get("d_model") is not None:
        if get("activation_function", "gelu") != "gelu":
            raise NotImplementedError(f"activation {get('activation_function')!r}: Whisper's erf GELU is what is built")
        size, ctx, width, heads, layers = (int(get(k)) for k in hf[:5])
        ffn = int(get(hf[5], 4 * width))
    else:
        raise ValueError(f"neither Whisper's ModelDimensions ({openai[2]} ...) nor a Hugging Face Whisper config (d_model ...)")
    return {first: size, "ctx": ctx, "width": width, "heads": heads, "layers": layers, "ffn": ffn}


# Hugging Face WhisperEncoder / WhisperDecoder names -> OpenAI's, applied in this order; then the side's final LayerNorm
_HF_TO_OPENAI = (("embed_positions.weight", "positional_embedding"), ("layers.", "blocks."), ("self_attn.q_proj", "attn.query"),
                 ("self_attn.k_proj", "attn.key"), ("self_attn.v_proj", "attn.value"), ("self_attn.out_proj", "attn.out"),
                 ("self_attn_layer_norm", "attn_ln"), ("final_layer_norm", "mlp_ln"), ("fc1", "mlp.0"), ("fc2", "mlp.2"))
_HF_TO_OPENAI_DEC = (("embed_tokens.weight", "token_embedding.weight"), ("embed_positions.weight", "positional_embedding"),
                     ("layers.", "blocks."), ("encoder_attn_layer_norm", "cross_attn_ln"), ("self_attn_layer_norm", "attn_ln"),
                     ("final_layer_norm", "mlp_ln"), ("encoder_attn.q_proj", "cross_attn.query"), ("encoder_attn.k_proj", "cross_attn.key"),
                     ("encoder_attn.v_proj", "cross_attn.value"), ("encoder_attn.out_proj", "cross_attn.out"),
                     ("self_attn.q_proj", "attn.query"), ("self_attn.k_proj", "attn.key"), ("self_attn.v_proj", "attn.value"),
                     ("self_attn.out_proj", "attn.out"), ("fc1", "mlp.0"), ("fc2", "mlp.2"))
_KEY_TABLES = {"audio": ("encoder.", _HF_TO_OPENAI, "ln_post."), "text": ("decoder.", _HF_TO_OPENAI_DEC, "ln.")}


def _canonical(state_dict: Dict[str, torch.Tensor], side: str = "audio") -> Dict[str, torch.Tensor]:
    """Either schema's tensors of one side under OpenAI's names without the ``encoder.`` / ``decoder.`` prefix.  Audio: decoder tensors
    are dropped and a key without a prefix counts as the encoder's (a bare WhisperEncoder state dict); text: everything that is not
    under ``decoder.`` is dropped."""
    prefix, table, final_ln = _KEY_TABLES[side]
    out = {}
    for k, v in state_dict.items():
        if k.startswith("model."):
            k = k[len("model."):]
        if k.startswith(prefix):
            k = k[len(prefix):]
        elif side == "text" or k.startswith("decoder.") or k.startswith("proj_out."):
            continue
        if k.startswith("layers.") or k.startswith("embed_") or k.startswith("layer_norm."):
            for a, b in table:
                k = k.replace(a, b)
            if k.startswith("layer_norm."):
                k = final_ln + k[len("layer_norm."):]
        out[k] = v
    return out


def _read_checkpoint(path: str, unresolved: str):
    """``path`` -> (``dims`` or config, state dict, whether it is a model directory): an OpenAI ``.pt`` (a dict with ``dims`` and
    ``model_state_dict``) or a Hugging Face model directory (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin``), picked by
    what ``path`` is.  Anything else, a model name included, raises FileNotFoundError ending in ``unresolved``: nothing is downloaded."""
    if os.path.isdir(path):
        with open(os.path.join(path, "config.json")) as f:
            return json.load(f), _load_weights(path), True
    if os.path.isfile(path):
        ckpt = torch.load(path, map_location="cpu")
        if not (isinstance(ckpt, dict) and "dims" in ckpt and "model_state_dict" in ckpt):
            raise ValueError(f"{path}: not a Whisper checkpoint (a dict with 'dims' and 'model_state_dict')")
        return ckpt["dims"], ckpt["model_state_dict"], False
    raise FileNotFoundError(f"{path!r} is neither a local .pt checkpoint nor a model directory{unresolved}")


class _FrozenWeights(nn.Module):
    """What ``AudioEncoder`` and ``TextDecoder`` share: the checkpoint's tensors as frozen fp32 parameters under OpenAI's names, and the
    cache of the fused operands (``prepared_weights()`` of the subclass), built on first use on a GPU and dropped on any move / cast."""

    def _freeze(self, sd: Dict[str, torch.Tensor], want: Dict[str, tuple]) -> None:
        for k, shape in want.items():
            if k not in sd:
                raise KeyError(f"{type(self).__name__}: {k} missing from the state dict")
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{type(self).__name__}: {k} has shape {tuple(sd[k].shape)}, expected {shape}")
            # parameter names cannot hold dots: keep the checkpoint's name with '/'
            self.register_parameter(k.replace(".", "/"), nn.Parameter(sd[k].detach().float().clone(), requires_grad=False))
        self._cache = None
        self._cache_kinds = {}

    # nn.Module plumbing: any move / cast invalidates the fused-weight cache, every kind of it together
    def _apply(self, fn, *a, **k):
        self._cache = None
        self._cache_kinds = {}
        return super()._apply(fn, *a, **k)

    def _p(self, name: str) -> torch.Tensor:
        return self._parameters[name.replace(".", "/")]

    @property
    def device(self) -> torch.device:
        return next(iter(self._parameters.values())).device

    def _require_gpu(self) -> None:
        if self.device.type != "cuda":
            raise RuntimeError(f"{_NAME}.{type(self).__name__} runs on MI355X only (no CPU fallback); move the model to a GPU")

    def _w(self):
        if self._cache is None:
            self._require_gpu()
            self._cache = self.prepared_weights()
        return self._cache

    def _w_kind(self, kind: str, prepare):
        """The preparation of a further kernel set (``AudioEncoder``: ``'x3'``) beside the fp32 one of ``_w()``: built once by
        ``prepare()``, kept next to it, dropped with it."""
        if kind not in self._cache_kinds:
            self._require_gpu()
            self._cache_kinds[kind] = prepare()
        return self._cache_kinds[kind]


_LN_EPS = 1e-5                 # of every LayerNorm of both halves


def _gemm(a_ptr, lda, w, bias, out_ptr, ldo, M, device, act=0, resid=None, periodic=None, period=0):
    """out[M, N] = act(A W^T + bias) (+ resid) (+ periodic[m % period]) on raw operand addresses: A's rows may overlap"""
    lib = _lib.load()
    N, K = w.shape
    ws, wsb = ops.stream_workspace(device, lib.hirest_gemm_f32_workspace_bytes(M, N, K))
    _lib.check(lib.hirest_gemm_f32_ws(a_ptr, lda, w.data_ptr(), K, bias.data_ptr(), resid.data_ptr() if resid is not None else None, N,
                                      periodic.data_ptr() if periodic is not None else None, period, out_ptr, ldo, M, N, K, act,
                                      ws, wsb, ops.stream_ptr()), "hirest_gemm_f32_ws")


def _linear(x, w, bias, act=0, resid=None):
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    _gemm(x.data_ptr(), x.shape[1], w, bias, out.data_ptr(), w.shape[0], x.shape[0], x.device, act=act, resid=resid)
    return out


def _ln_linear(x, gamma, beta, w, bias, act=0):
    """act(LayerNorm(x) W^T + bias): inside one GEMM where hirest_gemm_f32_ln has a form for the shape (up to 256 rows, K a multiple of
    256 up to 1024; from 8192 columns on — an LM head — only small.en's K = 768 up to 32 rows), else hirest_layernorm + hirest_gemm_f32:
    the same bits either way.  The condition is ``whisper_ln_gemm_fused`` of csrc/whisper_shared.h, its C twin behind the decode step and
    the prefill: the two have to stay the same.  No encoder product reaches 8192 columns (its N is 3 width, width or ffn)."""
    M, K = x.shape
    N = w.shape[0]
    if M <= 256 and K % 256 == 0 and K <= 1024 and (N < 8192 or (K == 768 and M <= 32)):
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().hirest_gemm_f32_ln(x.data_ptr(), K, None, None, None, gamma.data_ptr(), beta.data_ptr(), _LN_EPS, None, 0,
                                                  w.data_ptr(), K, bias.data_ptr(), None, 0, out.data_ptr(), N, M, N, K, act,
                                                  ops.stream_ptr()), "hirest_gemm_f32_ln")
        return out
    return _linear(ops.layernorm(x, gamma, beta, _LN_EPS, torch.empty_like(x)), w, bias, act=act)


class AudioEncoder(_FrozenWeights):
    """``whisper.model.AudioEncoder``: conv1 (k 3) + GELU, conv2 (k 3, stride 2) + GELU, + positional embedding, pre-LN blocks, ln_post.

    ``dims_or_config``: OpenAI's ``ModelDimensions`` / ``dims`` dict or a Hugging Face ``config.json`` dict; ``state_dict`` in either
    schema (``encoder.blocks.i.attn.query ...`` or ``[model.]encoder.layers.i.self_attn.q_proj ...``; decoder tensors are ignored).
    The weights are frozen parameters under OpenAI's names; the fused operands are built on first use and dropped on any move / cast.

    ``set_precision("bf16x3")`` runs the blocks and ``ln_post`` on split operands (csrc/whisper_enc_x3.hip: every weight product and both
    attention products from bf16 hi + lo splits, three bf16 MFMAs each, fp32 accumulation; residual stream, LayerNorm and softmax fp32);
    the stem stays exact fp32 in both.  The default, ``"fp32"``, is exact fp32 throughout.  What is set is what runs, at every batch size."""

    PRECISIONS = ("fp32", "bf16x3")

    def __init__(self, dims_or_config, state_dict: Dict[str, torch.Tensor]):
        super().__init__()
        self._precision = "fp32"
        self.dims = _dims(dims_or_config, "audio")
        d = self.dims
        self.n_mels, self.ctx, self.width, self.heads, self.layers, self.ffn = (d[k] for k in ("n_mels", "ctx", "width", "heads", "layers", "ffn"))
        if self.width % self.heads or self.width % 16 or self.ffn % 16 or self.n_mels % 16:
            raise NotImplementedError(f"width {self.width} / heads {self.heads} / ffn {self.ffn} / n_mels {self.n_mels}: multiples of 16 expected")
        self.dh = self.width // self.heads
        if self.dh > _AH_MAX:
            raise NotImplementedError(f"head width {self.dh} > {_AH_MAX}")
        self.ah = _padded_head_width(self.heads, self.dh)
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
        self._freeze(_canonical(state_dict, "audio"), want)

    def prepared_weights(self) -> Dict[str, torch.Tensor]:
        """The operands the kernels read, on the parameters' device: reordered convolution weights, per-block fused QKV (zero key bias,
        heads zero-padded to the attention kernel's width) and output projections."""
        f = lambda n: self._p(n).detach().float().contiguous()
        c = {"conv1_w": conv_as_gemm_weight(f("conv1.weight")), "conv1_b": f("conv1.bias"),
             "conv2_w": conv_as_gemm_weight(f("conv2.weight")), "conv2_b": f("conv2.bias"),
             "pos": f("positional_embedding"), "ln_post_w": f("ln_post.weight"), "ln_post_b": f("ln_post.bias")}
        no_bias = torch.zeros(self.width, device=self.device)
        for i in range(self.layers):
            p = f"blocks.{i}."
            c[f"qkv_w.{i}"], c[f"qkv_b.{i}"], c[f"o_w.{i}"] = _fused_head_operands(
                [(f(p + f"attn.{n}.weight"), f(p + f"attn.{n}.bias") if n != "key" else no_bias) for n in ("query", "key", "value")],
                f(p + "attn.out.weight"), self.heads, self.dh, self.ah)
            for n in ("attn.out.bias", "attn_ln.weight", "attn_ln.bias", "mlp_ln.weight", "mlp_ln.bias", "mlp.0.weight", "mlp.0.bias",
                      "mlp.2.weight", "mlp.2.bias"):
                c[p + n] = f(p + n)
        return c

    @property
    def precision(self) -> str:
        return self._precision

    def set_precision(self, precision: str) -> "AudioEncoder":
        """``"fp32"`` (default) or ``"bf16x3"``.  Prepares nothing and needs no GPU: the operands of a precision are built on its first
        use and stay resident beside the other's."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision {precision!r}: one of {', '.join(self.PRECISIONS)} expected")
        if precision == "bf16x3" and (self.width % 32 or self.ffn % 32):
            raise NotImplementedError(f"bf16x3: width {self.width} / ffn {self.ffn} are not multiples of 32 (the split operand's blocks)")
        self._precision = precision
        return self

    def prepared_weights_x3(self) -> Dict[str, object]:
        """The descriptor of csrc/whisper_enc_x3.hip (``hirest_whisper_encoder_x3``): per block the four weights split into bf16 hi | lo
        (``ops.split2``; the fused query | key | value with a zero key bias and NO head padding — the split-operand attention takes the
        head width as it is), the fp32 LayerNorm and bias vectors of the fp32 preparation, and ``ln_post``."""
        c = self._w()
        f = lambda n: self._p(n).detach().float().contiguous()
        keep, layers = [], (_lib.WhisperLayerX3 * self.layers)()
        no_bias = torch.zeros(self.width, device=self.device)
        for i in range(self.layers):
            p = f"blocks.{i}."
            qkv_w2 = ops.split2(torch.cat([f(p + f"attn.{n}.weight") for n in ("query", "key", "value")]))
            qkv_b = torch.cat([f(p + "attn.query.bias"), no_bias, f(p + "attn.value.bias")])
            out_w2, fc1_w2, fc2_w2 = (ops.split2(f(p + n)) for n in ("attn.out.weight", "mlp.0.weight", "mlp.2.weight"))
            t = {"attn_ln_g": c[p + "attn_ln.weight"], "attn_ln_b": c[p + "attn_ln.bias"], "qkv_w2": qkv_w2, "qkv_b": qkv_b,
                 "out_w2": out_w2, "out_b": c[p + "attn.out.bias"], "mlp_ln_g": c[p + "mlp_ln.weight"], "mlp_ln_b": c[p + "mlp_ln.bias"],
                 "fc1_w2": fc1_w2, "fc1_b": c[p + "mlp.0.bias"], "fc2_w2": fc2_w2, "fc2_b": c[p + "mlp.2.bias"]}
            keep.append(t)                                           # (the device tensors behind the raw pointers)
            for name, v in t.items():
                setattr(layers[i], name, v.data_ptr())
        desc = _lib.WhisperEncoderX3(struct_size=C.sizeof(_lib.WhisperEncoderX3), layers=self.layers, heads=self.heads, width=self.width,
                                     ffn=self.ffn, ctx=self.ctx, flags=0, ln_eps=_LN_EPS, layer=layers,
                                     ln_post_g=c["ln_post_w"].data_ptr(), ln_post_b=c["ln_post_b"].data_ptr())
        return {"desc": desc, "layers": layers, "keep": keep, "fp32": c}

    def _blocks_x3(self, x: torch.Tensor, B: int) -> torch.Tensor:
        """The blocks and ln_post of ``x`` [B ctx, width] in one C call; its scratch is per stream (``ops.stream_workspace``)"""
        lib = _lib.load()
        desc = C.byref(self._w_kind("x3", self.prepared_weights_x3)["desc"])
        need = lib.hirest_whisper_encoder_x3_workspace_bytes(desc, B)
        if need == 0:
            raise NotImplementedError(f"bf16x3: no kernel for width {self.width} / heads {self.heads} / ffn {self.ffn}")
        ws, wsb = ops.stream_workspace(x.device, need, "whisper_encoder_x3")
        out = torch.empty_like(x)
        _lib.check(lib.hirest_whisper_encoder_x3_forward(desc, x.data_ptr(), B, out.data_ptr(), ws, wsb, ops.stream_ptr()),
                   "hirest_whisper_encoder_x3_forward")
        return out

    # ------------------------------------------------------------------------------------------------------------

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
            _gemm(rows[b].data_ptr(), C, c["conv1_w"], c["conv1_b"], h[b, 1].data_ptr(), D, T, dev, act=1)
            # conv2 (stride 2): output row t reads padded rows 2 t, 2 t + 1, 2 t + 2; GELU, then + positional embedding (row t of the clip)
            _gemm(h[b].data_ptr(), 2 * D, c["conv2_w"], c["conv2_b"], x[b * ctx].data_ptr(), D, ctx, dev, act=1,
                       periodic=c["pos"], period=ctx)
        return x

    @torch.no_grad()
    def forward(self, mel: torch.Tensor, return_stem: bool = False) -> torch.Tensor:
        """``mel`` ``[B, n_mels, 2 ctx]`` or ``[n_mels, 2 ctx]`` -> ``[B, ctx, width]`` fp32 encoder states (``return_stem``: the input of
        the first block instead).  Any other frame count raises ValueError, where Whisper asserts."""
        self._require_gpu()
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
            if self._precision == "bf16x3":
                return self._blocks_x3(x, B).view(B, ctx, self.width)
            for i in range(self.layers):
                p = f"blocks.{i}."
                qkv = _ln_linear(x, c[p + "attn_ln.weight"], c[p + "attn_ln.bias"], c[f"qkv_w.{i}"], c[f"qkv_b.{i}"])
                att = torch.empty((B * ctx, H * AH), dtype=torch.float32, device=dev)
                _lib.check(lib.hirest_attention_f32(qkv.data_ptr(), att.data_ptr(), B, ctx, H, AH, self.dh ** -0.5, 0.0, ops.stream_ptr()),
                           "hirest_attention_f32")
                x = _linear(att, c[f"o_w.{i}"], c[p + "attn.out.bias"], resid=x)
                hid = _ln_linear(x, c[p + "mlp_ln.weight"], c[p + "mlp_ln.bias"], c[p + "mlp.0.weight"], c[p + "mlp.0.bias"], act=1)
                x = _linear(hid, c[p + "mlp.2.weight"], c[p + "mlp.2.bias"], resid=x)
            out = ops.layernorm(x, c["ln_post_w"], c["ln_post_b"], _LN_EPS, torch.empty_like(x))
        return out.view(B, ctx, self.width)

    embed_audio = forward


def _load_precision(precision: Optional[str]) -> str:
    """The encoder precision of a load: the keyword, else ``HIREST_WHISPER_PRECISION`` (so that an unmodified driver reaches the mode, as
    ``HIREST_PRECISION`` does for the towers), else ``"fp32"``"""
    return precision if precision is not None else (os.environ.get("HIREST_WHISPER_PRECISION") or "fp32")


def load_encoder(path: str, device: Optional[Union[str, torch.device]] = None, *, precision: Optional[str] = None) -> AudioEncoder:
    """An OpenAI ``.pt`` checkpoint (a dict with ``dims`` and ``model_state_dict``) or a Hugging Face model directory (``config.json`` +
    ``model.safetensors`` / ``pytorch_model.bin``), picked by what ``path`` is.  A model name (``'small.en'``, ``'openai/whisper-small.en'``)
    raises FileNotFoundError: nothing is downloaded.  ``precision``: ``AudioEncoder.set_precision``'s (default: the environment's
    ``HIREST_WHISPER_PRECISION``, else ``"fp32"``); a bad name raises ValueError here."""
    dims, sd, _ = _read_checkpoint(path, " (no network access: download the model beforehand and pass its path)")
    enc = AudioEncoder(dims, sd).set_precision(_load_precision(precision))
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


# ---------------------------------------------------------------------------------------------------------------------------------
# the text decoder
# ---------------------------------------------------------------------------------------------------------------------------------

_CAUSAL_PENALTY = -1.0e30      # added to scores of future keys in prefill: exp() of it is exactly 0 against any fp32 score, no overflow


PREFILL_ROWS_PER_CALL = 4096   # packed prompt rows of one hirest_whisper_prefill_rows call: bounds its workspace


def prefill_plan(prompts, first_rows, groups, windows, sot_indices=None, rows_per_call: int = PREFILL_ROWS_PER_CALL):
    """The ``hirest_whisper_prefill_seq`` tables of ``TextDecoder.prefill_many``, a pure function: a list of calls, each a list of
    ``(offset, length, window, first_row, n_rows, sot_index)`` in the prompts' order.  Offsets restart at 0 in every call; a call
    takes consecutive prompts while they fit ``rows_per_call`` packed rows (at least one).  ``sot_index`` is -1 where none is given
    or where it is the last position, whose logits are returned anyway."""
    n = len(prompts)
    sot_indices = [None] * n if sot_indices is None else list(sot_indices)
    if not (len(first_rows) == len(groups) == len(windows) == len(sot_indices) == n) or n == 0:
        raise ValueError("prefill_plan: one first row, group, window and sot index per prompt, and at least one prompt")
    calls, cur, off = [], [], 0
    for p, r0, g, w, sot in zip(prompts, first_rows, groups, windows, sot_indices):
        T = len(p)
        if T < 1:
            raise ValueError("prefill_plan: an empty prompt")
        if sot is not None and not 0 <= sot < T:
            raise ValueError(f"prefill_plan: sot index {sot} outside a prompt of {T} tokens")
        if cur and off + T > rows_per_call:
            calls.append(cur)
            cur, off = [], 0
        cur.append((off, T, int(w), int(r0), int(g), -1 if sot is None or sot == T - 1 else int(sot)))
        off += T
    calls.append(cur)
    return calls


def window_row_ranges(row_window: Sequence[int], n_windows: int) -> List[Tuple[int, int]]:
    """``row_window [R]`` -> per window (first row, row count); ValueError where a window's rows are not contiguous, where a window
    has no row, or where a row names a window outside ``[0, n_windows)``."""
    ranges = [None] * n_windows
    for r, w in enumerate(row_window):
        if not 0 <= w < n_windows:
            raise ValueError(f"row {r} names window {w} of {n_windows}")
        if ranges[w] is None:
            ranges[w] = (r, 1)
        elif ranges[w][0] + ranges[w][1] == r:
            ranges[w] = (ranges[w][0], ranges[w][1] + 1)
        else:
            raise ValueError(f"the rows of window {w} are not contiguous (row {r} after row {ranges[w][0] + ranges[w][1] - 1})")
    for w, rg in enumerate(ranges):
        if rg is None:
            raise ValueError(f"window {w} has no row")
    return ranges


def _seq_table(seqs):
    table = (_lib.WhisperPrefillSeq * len(seqs))()
    for t, (off, T, w, r0, g, sot) in zip(table, seqs):
        t.offset, t.length, t.window, t.first_row, t.n_rows, t.sot_index = off, T, w, r0, g, sot
    return table


class KVCache:
    """What a decoding loop keeps between steps: per layer the preallocated self-attention cache ``[R, T_max, D]`` (key, value), the
    cross-attention ``key(xa) | value(xa)`` rows ``[n_windows, Tk, 2 D]``, ``row_window [R]`` and the number of filled positions.
    ``per_row``: the rows sit at positions of their own (``TextDecoder.step_rows``: ``detect_language``, and the decoding loop's
    ``DecodeState``): the workspace is ``hirest_whisper_decode_step_rows``'s and ``length`` is not used."""

    def __init__(self, decoder: "TextDecoder", xa: torch.Tensor, row_window: torch.Tensor, T_max: Optional[int] = None, per_row: bool = False):
        self._allocate(decoder, int(row_window.numel()), int(xa.shape[0]), int(xa.shape[1]), int(T_max or decoder.ctx), per_row)
        self.load(decoder, xa, row_window)

    def _allocate(self, decoder: "TextDecoder", R: int, n_windows: int, Tk: int, T_max: int, per_row: bool) -> None:
        dev, D, L = decoder.device, decoder.width, decoder.layers
        self.R, self.T_max, self.length, self.n_windows, self.Tk = R, T_max, 0, n_windows, Tk
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self.row_window = torch.empty((R,), dtype=torch.int32, device=dev)
        self.self_k, self.self_v = [f32(R, T_max, D) for _ in range(L)], [f32(R, T_max, D) for _ in range(L)]
        self.cross_kv = [f32(n_windows, Tk, 2 * D) for _ in range(L)]
        P = C.c_void_p * L
        self.k_ptrs, self.v_ptrs = P(*(t.data_ptr() for t in self.self_k)), P(*(t.data_ptr() for t in self.self_v))
        self.x_ptrs = P(*(t.data_ptr() for t in self.cross_kv))
        self.logits = f32(R, decoder.vocab_padded)
        lib = _lib.load()
        need = (lib.hirest_whisper_step_rows_workspace_bytes if per_row else lib.hirest_whisper_step_workspace_bytes)(
            C.byref(decoder._w()["desc"]), R, Tk)
        self.ws = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=dev)

    def load(self, decoder: "TextDecoder", xa: torch.Tensor, row_window: torch.Tensor) -> None:
        """a loop's windows: ``row_window`` and every layer's cross key | value rows, computed into the cache's own buffers"""
        self.row_window.copy_(row_window)
        decoder.cross_kv(xa, self.cross_kv)


class DecodeState(KVCache):
    """Everything a per-row decoding loop reads and writes between its prefill and its read-back: a per-row ``KVCache`` of ``T_max``
    positions, and the rows' records (``ctl``), states, next ids, tokens ``[R, slots]``, the suppress mask, the counted tail's call
    counter and the pinned stamp.  The eager loop makes one per loop, as large as its prompts and step budgets need; the replayed loop
    keeps one per shape at the decoder's whole context (``_decode_arena``: addresses that do not change from loop to loop), whose
    ``graph`` is the captured chunk and ``graph_key`` what it was captured with: another key captures again."""

    def __init__(self, decoder: "TextDecoder", R: int, n_windows: int, Tk: int, T_max: int, slots: int):
        self._allocate(decoder, R, n_windows, Tk, T_max, per_row=True)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=decoder.device)
        self.ctl, self.state = i32(R, _lib.WHISPER_ROW_CTL_WORDS), i32(R, _lib.WHISPER_ROW_STATE_WORDS)
        self.ids, self.tokens = i32(R), i32(R, slots)
        self.mask, self.count = i32((decoder.vocab_padded + 31) // 32), i32(1)
        self.stamp = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.stamp_host = self.stamp.numpy()                          # the same word, read without a tensor per poll
        self.graph, self.graph_key = None, None

    def reset(self, ctl_rows, eot: int, last: torch.Tensor) -> None:
        """a loop's rows: their records from ``(position, step, max_steps, draw_row, seed, temperature)`` per row, a fresh state, no
        token yet, and as first logits the last prompt position's of each row's window (``last [n_windows, vocab_padded]``)"""
        self.ctl.copy_(new_row_ctl(ctl_rows, "cpu"))
        self.state.copy_(new_row_state(self.R, "cpu"))
        self.tokens.fill_(eot)
        self.ids.zero_()
        torch.index_select(last, 0, self.row_window, out=self.logits)      # every iteration reads its logits at the same address
        self.stamp_host[0] = 0                                        # (the loop before this one ended with a synchronisation)

    def tail(self, params, call: Optional[int] = None, stream=None) -> None:
        """The rows' next tokens from ``logits``: with ``call``, the loop's call number, ``hirest_whisper_step_tail_rows``; without, the
        counted entry, which keeps that number on the device (``count``) so that a captured launch serves every call."""
        lib, Vp = _lib.load(), int(self.logits.shape[1])
        rest = (int(self.tokens.shape[1]), C.byref(params), self.ctl.data_ptr(), self.state.data_ptr(), self.ids.data_ptr(),
                self.tokens.data_ptr(), None, self.stamp.data_ptr(), ops.stream_ptr() if stream is None else stream)
        if call is None:
            _lib.check(lib.hirest_whisper_step_tail_rows_counted(self.logits.data_ptr(), Vp, self.R, Vp, self.count.data_ptr(), *rest),
                       "hirest_whisper_step_tail_rows_counted")
        else:
            _lib.check(lib.hirest_whisper_step_tail_rows(self.logits.data_ptr(), Vp, self.R, Vp, call, *rest), "hirest_whisper_step_tail_rows")


class TextDecoder(_FrozenWeights):
    """``whisper.model.TextDecoder``: token + learned positional embedding, pre-LN blocks (self-attention, cross-attention over the audio
    encoder's states, MLP), ``ln``, the tied-embedding LM head.  ``dims_or_config`` / ``state_dict`` as ``AudioEncoder``'s (either schema).

    ``forward(tokens, xa)`` runs whole sequences (teacher forcing, a window's prompt) through the full-sequence kernels.  With a
    ``KVCache`` it fills the cache from a prompt shared by all rows (``tokens [1, T]`` or ``[T]``; the cache rows are broadcast) — over
    several windows from one prompt per window (``tokens [n_windows, T]``, Whisper's batched call) — or, once the cache holds
    positions, takes one new token per row (``tokens [R, 1]``) through ``hirest_whisper_decode_step``.  ``prefill_many`` is the decoding
    loop's prefill: prompts of different lengths for all its windows in one ``hirest_whisper_prefill_rows`` call."""

    def __init__(self, dims_or_config, state_dict: Dict[str, torch.Tensor]):
        super().__init__()
        self.dims = _dims(dims_or_config, "text")
        d = self.dims
        self.vocab, self.ctx, self.width, self.heads, self.layers, self.ffn = (d[k] for k in ("vocab", "ctx", "width", "heads", "layers", "ffn"))
        if self.width != 64 * self.heads:
            raise NotImplementedError(f"width {self.width} / heads {self.heads}: 64-wide heads (every Whisper size) are what is built")
        if self.ffn % 16:
            raise NotImplementedError(f"ffn {self.ffn}: a multiple of 16 expected")
        self.vocab_padded = (self.vocab + 3) // 4 * 4
        self.graph_stats = {"captures": 0, "replays": 0, "eager_steps": 0}          # Whisper.graph_stats()
        D, I = self.width, self.ffn
        want = {"token_embedding.weight": (self.vocab, D), "positional_embedding": (self.ctx, D), "ln.weight": (D,), "ln.bias": (D,)}
        for i in range(self.layers):
            p = f"blocks.{i}."
            for a in ("attn", "cross_attn"):
                for n in ("query", "key", "value", "out"):
                    want[p + f"{a}.{n}.weight"] = (D, D)
                    if n != "key":
                        want[p + f"{a}.{n}.bias"] = (D,)
                want[p + f"{a}_ln.weight"] = want[p + f"{a}_ln.bias"] = (D,)
            want.update({p + "mlp_ln.weight": (D,), p + "mlp_ln.bias": (D,), p + "mlp.0.weight": (I, D), p + "mlp.0.bias": (I,),
                         p + "mlp.2.weight": (D, I), p + "mlp.2.bias": (D,)})
        self._freeze(_canonical(state_dict, "text"), want)

    def prepared_weights(self) -> Dict[str, object]:
        """The operands the kernels read: fused query | key | value (zero key bias), fused cross key | value, the embedding zero-padded to a
        multiple of 4 rows (also the LM head) with a zero bias, and the C descriptor over them (``desc``)."""
        f = lambda n: self._p(n).detach().float().contiguous()
        D, dev = self.width, self.device
        z = torch.zeros(D, device=dev)
        emb = torch.zeros((self.vocab_padded, D), device=dev)
        emb[:self.vocab] = f("token_embedding.weight")
        c = {"tok": emb, "pos": f("positional_embedding"), "ln_g": f("ln.weight"), "ln_b": f("ln.bias"),
             "lm_b": torch.zeros(self.vocab_padded, device=dev)}
        layers = (_lib.WhisperLayer * self.layers)()
        for i in range(self.layers):
            p = f"blocks.{i}."
            c[f"qkv_w.{i}"] = torch.cat([f(p + f"attn.{n}.weight") for n in ("query", "key", "value")], 0).contiguous()
            c[f"qkv_b.{i}"] = torch.cat([f(p + "attn.query.bias"), z, f(p + "attn.value.bias")], 0).contiguous()
            c[f"ckv_w.{i}"] = torch.cat([f(p + "cross_attn.key.weight"), f(p + "cross_attn.value.weight")], 0).contiguous()
            c[f"ckv_b.{i}"] = torch.cat([z, f(p + "cross_attn.value.bias")], 0).contiguous()
            for n in ("attn.out.weight", "attn.out.bias", "attn_ln.weight", "attn_ln.bias", "cross_attn_ln.weight", "cross_attn_ln.bias",
                      "cross_attn.query.weight", "cross_attn.query.bias", "cross_attn.out.weight", "cross_attn.out.bias", "mlp_ln.weight",
                      "mlp_ln.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"):
                c[p + n] = f(p + n)
            L = layers[i]
            for field, key in (("attn_ln_g", p + "attn_ln.weight"), ("attn_ln_b", p + "attn_ln.bias"), ("qkv_w", f"qkv_w.{i}"), ("qkv_b", f"qkv_b.{i}"),
                               ("so_w", p + "attn.out.weight"), ("so_b", p + "attn.out.bias"), ("cross_ln_g", p + "cross_attn_ln.weight"),
                               ("cross_ln_b", p + "cross_attn_ln.bias"), ("cq_w", p + "cross_attn.query.weight"),
                               ("cq_b", p + "cross_attn.query.bias"), ("co_w", p + "cross_attn.out.weight"), ("co_b", p + "cross_attn.out.bias"),
                               ("mlp_ln_g", p + "mlp_ln.weight"), ("mlp_ln_b", p + "mlp_ln.bias"), ("fc1_w", p + "mlp.0.weight"),
                               ("fc1_b", p + "mlp.0.bias"), ("fc2_w", p + "mlp.2.weight"), ("fc2_b", p + "mlp.2.bias")):
                setattr(L, field, c[key].data_ptr())
        desc = _lib.WhisperDecoder()
        desc.layers, desc.heads, desc.hidden, desc.inter, desc.vocab_padded, desc.max_pos = (self.layers, self.heads, D, self.ffn, self.vocab_padded,
                                                                                               self.ctx)
        desc.tok_emb, desc.pos_emb, desc.layer = c["tok"].data_ptr(), c["pos"].data_ptr(), layers
        desc.ln_g, desc.ln_b, desc.lm_b = c["ln_g"].data_ptr(), c["ln_b"].data_ptr(), c["lm_b"].data_ptr()
        c["layers"], c["desc"] = layers, desc
        return c

    @torch.no_grad()
    def cross_kv(self, xa: torch.Tensor, out: Optional[List[torch.Tensor]] = None):
        """``xa [n_windows, Tk, D]`` -> per layer ``[n_windows, Tk, 2 D]``: the layer's ``key(xa) | value(xa)``, computed once per window;
        into ``out``'s tensors where they are given"""
        c, dev = self._w(), self.device
        W, Tk, D = xa.shape
        rows = xa.to(dev, torch.float32).contiguous().view(W * Tk, D)
        with torch.cuda.device(dev):
            if out is None:
                out = [torch.empty((W, Tk, 2 * D), dtype=torch.float32, device=dev) for _ in range(self.layers)]
            for i, kv in enumerate(out):
                _gemm(rows.data_ptr(), D, c[f"ckv_w.{i}"], c[f"ckv_b.{i}"], kv.data_ptr(), 2 * D, W * Tk, dev)
        return out

    def _sequences(self, tokens: torch.Tensor, cross_kv, Tk: int, keep=None, keep_cross_q=None):
        """[B, T] tokens (sequence b against window b of cross_kv) -> [B * T, D] states before ``ln``; ``keep(i, qkv)`` sees every layer's
        packed q | k | v rows (the prefill takes its cache rows from them), ``keep_cross_q(i, q)`` every layer's cross-attention query
        rows ``[B * T, D]`` (the word alignment takes its attention weights from them); without them nothing is kept"""
        c, lib = self._w(), _lib.load()
        B, T = tokens.shape
        D, H, dev = self.width, self.heads, self.device
        ids = tokens.to(dev, torch.int32).contiguous().view(-1)
        x = torch.empty((B * T, D), dtype=torch.float32, device=dev)
        _lib.check(lib.hirest_embedding_fwd_f32(ids.data_ptr(), c["tok"].data_ptr(), c["pos"].data_ptr(), x.data_ptr(), B * T, T, D,
                                                ops.stream_ptr()), "hirest_embedding_fwd_f32")
        for i in range(self.layers):
            p = f"blocks.{i}."
            qkv = _ln_linear(x, c[p + "attn_ln.weight"], c[p + "attn_ln.bias"], c[f"qkv_w.{i}"], c[f"qkv_b.{i}"])
            if keep is not None:
                keep(i, qkv)
            att = torch.empty((B * T, D), dtype=torch.float32, device=dev)
            _lib.check(lib.hirest_attention_f32_qkv(qkv.data_ptr(), 3 * D, qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, att.data_ptr(), B, T,
                                                    T, H, 64, 0.125, 0.0, _CAUSAL_PENALTY, ops.stream_ptr()), "hirest_attention_f32_qkv")
            x = _linear(att, c[p + "attn.out.weight"], c[p + "attn.out.bias"], resid=x)
            q = _ln_linear(x, c[p + "cross_attn_ln.weight"], c[p + "cross_attn_ln.bias"], c[p + "cross_attn.query.weight"],
                           c[p + "cross_attn.query.bias"])
            if keep_cross_q is not None:
                keep_cross_q(i, q)
            kv = cross_kv[i]
            _lib.check(lib.hirest_attention_f32_qkv(q.data_ptr(), D, kv.data_ptr(), kv.data_ptr() + 4 * D, 2 * D, att.data_ptr(), B, T, Tk, H, 64,
                                                    0.125, 0.0, 0.0, ops.stream_ptr()), "hirest_attention_f32_qkv")
            x = _linear(att, c[p + "cross_attn.out.weight"], c[p + "cross_attn.out.bias"], resid=x)
            hid = _ln_linear(x, c[p + "mlp_ln.weight"], c[p + "mlp_ln.bias"], c[p + "mlp.0.weight"], c[p + "mlp.0.bias"], act=1)
            x = _linear(hid, c[p + "mlp.2.weight"], c[p + "mlp.2.bias"], resid=x)
        return x

    def _head(self, x: torch.Tensor) -> torch.Tensor:
        c = self._w()
        return _ln_linear(x, c["ln_g"], c["ln_b"], c["tok"], c["lm_b"])

    @torch.no_grad()
    def forward(self, tokens: torch.Tensor, xa: Optional[torch.Tensor], kv_cache: Optional[KVCache] = None) -> torch.Tensor:
        """``tokens [B, T]``, ``xa [B, Tk, D]`` -> logits ``[B, T, n_vocab]``.  With ``kv_cache`` (``xa`` is then the cache's own): an empty
        cache over one window takes the shared prompt ``[1, T]`` and returns ``[1, T, n_vocab]``, one over several windows takes a
        prompt per window ``[n_windows, T]`` and returns ``[n_windows, T, n_vocab]``; a filled one takes ``[R, 1]`` and returns
        ``[R, 1, n_vocab]``."""
        self._require_gpu()
        if tokens.ndim == 1:
            tokens = tokens[None]
        B, T = tokens.shape
        with torch.cuda.device(self.device):
            if kv_cache is None:
                if xa is None or xa.ndim != 3 or xa.shape[0] != B or xa.shape[2] != self.width:
                    raise ValueError(f"xa of shape {None if xa is None else tuple(xa.shape)}: [{B}, Tk, {self.width}] expected")
                if T > self.ctx:
                    raise ValueError(f"{T} tokens: the decoder has {self.ctx} positions")
                x = self._sequences(tokens, self.cross_kv(xa), int(xa.shape[1]))
                return self._head(x).view(B, T, self.vocab_padded)[..., :self.vocab]
            kc = kv_cache
            if kc.length == 0:
                if kc.n_windows == 1 and B != 1:
                    raise ValueError("an empty cache is filled from ONE prompt shared by its rows: tokens [1, T]")
                if kc.n_windows > 1 and B != kc.n_windows:
                    raise ValueError(f"an empty cache over {kc.n_windows} windows is filled from one prompt per window: tokens [{kc.n_windows}, T]")
                return self.prefill(tokens, kc).view(B, T, self.vocab_padded)[..., :self.vocab]
            if T != 1 or B != kc.R:
                raise ValueError(f"a filled cache takes one new token per row: tokens [{kc.R}, 1]")
            self.step(tokens.to(self.device, torch.int32).contiguous().view(-1), kc)
            return kc.logits.view(B, 1, self.vocab_padded)[..., :self.vocab]

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, kc: KVCache, rows: Optional[slice] = None, window: Optional[int] = None) -> torch.Tensor:
        """The prompt ``[1, T]`` shared by every row of an empty cache, once: fills positions 0 .. T - 1 of all rows' caches (broadcast),
        sets ``kc.length`` and returns the prompt's logits ``[T, vocab_padded]``.  With ``window`` (the decoding loop's per-row cache over
        several windows): the same for the slice ``rows`` against that window's cross keys / values; ``kc.length`` stays.  Without
        ``window`` on a cache over several windows: ``tokens [n_windows, T]``, prompt w for every row with ``row_window == w`` (a
        window's rows must be contiguous: ValueError otherwise); returns ``[n_windows * T, vocab_padded]``."""
        T = int(tokens.shape[-1])
        if kc.length != 0:
            raise ValueError("prefill of a cache that already holds positions")
        if T > min(kc.T_max, self.ctx):
            raise ValueError(f"a prompt of {T} tokens does not fit the cache's {kc.T_max} positions")
        D = self.width
        if window is None and kc.n_windows != 1:
            if tokens.ndim != 2 or tokens.shape[0] != kc.n_windows:
                raise ValueError(f"tokens of shape {tuple(tokens.shape)}: one prompt per window, [{kc.n_windows}, T], expected")
            ranges = window_row_ranges(kc.row_window.tolist(), kc.n_windows)          # (a read-back; this is not the loop's path)
            seqs = prefill_plan([[0] * T] * kc.n_windows, [r0 for r0, _ in ranges], [n for _, n in ranges], range(kc.n_windows),
                                rows_per_call=kc.n_windows * T)[0]
            table = _seq_table(seqs)

            def scatter(i, qkv):       # every window's keys / values into its rows, one launch per layer
                _lib.check(_lib.load().hirest_whisper_prefill_scatter(qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, kc.self_k[i].data_ptr(),
                                                                      kc.self_v[i].data_ptr(), kc.R, kc.T_max, D, table, len(seqs), ops.stream_ptr()),
                           "hirest_whisper_prefill_scatter")
            with torch.cuda.device(self.device):
                x = self._sequences(tokens, kc.cross_kv, kc.Tk, scatter)
                kc.length = T
                return self._head(x)
        w, rows = window or 0, rows if rows is not None else slice(None)

        def keep(i, qkv):          # the prompt's keys / values, the same for every candidate row of the window
            kc.self_k[i][rows, :T] = qkv[:, D:2 * D]
            kc.self_v[i][rows, :T] = qkv[:, 2 * D:]
        with torch.cuda.device(self.device):
            x = self._sequences(tokens.view(1, T), [kv[w:w + 1] for kv in kc.cross_kv], kc.Tk, keep)
            if window is None:
                kc.length = T
            return self._head(x)

    @torch.no_grad()
    def prefill_many(self, prompts: Sequence[Sequence[int]], kc: KVCache, first_rows: Sequence[int], groups: Sequence[int],
                     windows: Sequence[int], sot_indices: Optional[Sequence[Optional[int]]] = None, rows_per_call: Optional[int] = None):
        """The decoding loop's prefill: prompt s (a list of token ids, each of its own length) against window ``windows[s]``'s cross
        keys / values fills positions ``0 .. len - 1`` of cache rows ``first_rows[s] .. first_rows[s] + groups[s] - 1`` — all prompts
        as packed rows through ONE ``hirest_whisper_prefill_rows`` call (consecutive calls past ``rows_per_call`` packed rows,
        ``PREFILL_ROWS_PER_CALL`` unless given), with the bits of ``prefill(tokens[1, T], kc, rows=, window=)`` prompt by prompt.  -> ``(logits_last [n_seq,
        vocab_padded], logits_sot)``: the logits of every prompt's last position and, where ``sot_indices[s]`` names another position,
        of that one (``None`` when no prompt does; rows of the others are not written).  ``kc.length`` stays."""
        limit = min(kc.T_max, self.ctx)
        for p in prompts:
            if not 1 <= len(p) <= limit:
                raise ValueError(f"a prompt of {len(p)} tokens does not fit the cache's {kc.T_max} positions (the decoder has {self.ctx})")
        calls = prefill_plan(prompts, first_rows, groups, windows, sot_indices, rows_per_call or PREFILL_ROWS_PER_CALL)
        lib, dev, Vp = _lib.load(), self.device, self.vocab_padded
        desc = C.byref(self._w()["desc"])
        with torch.cuda.device(dev):
            last = torch.empty((len(prompts), Vp), dtype=torch.float32, device=dev)
            sot = torch.empty((len(prompts), Vp), dtype=torch.float32, device=dev) if any(q[5] >= 0 for c in calls for q in c) else None
            ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32).to(dev)
            s0 = n0 = 0
            for seqs in calls:
                N = sum(q[1] for q in seqs)
                ws = torch.empty((max(int(lib.hirest_whisper_prefill_workspace_bytes(desc, N, len(seqs))), 1),), dtype=torch.uint8, device=dev)
                _lib.check(lib.hirest_whisper_prefill_rows(desc, len(seqs), _seq_table(seqs), ids.data_ptr() + 4 * n0, kc.k_ptrs, kc.v_ptrs, kc.R,
                                                           kc.T_max, kc.x_ptrs, kc.n_windows, kc.Tk, last.data_ptr() + 4 * Vp * s0,
                                                           sot.data_ptr() + 4 * Vp * s0 if sot is not None else None, ws.data_ptr(), ws.numel(),
                                                           ops.stream_ptr()), "hirest_whisper_prefill_rows")
                s0, n0 = s0 + len(seqs), n0 + N
        return last, sot

    def step(self, ids: torch.Tensor, kc: KVCache) -> torch.Tensor:
        """one position for every row of the cache: ``ids`` int32 ``[R]`` on the device -> ``kc.logits [R, vocab_padded]``"""
        if kc.length >= min(kc.T_max, self.ctx):
            raise ValueError(f"position {kc.length}: the cache holds {kc.T_max} positions, the decoder {self.ctx}")
        _lib.check(_lib.load().hirest_whisper_decode_step(C.byref(self._w()["desc"]), kc.R, kc.length, ids.data_ptr(), kc.k_ptrs, kc.v_ptrs, kc.T_max,
                                                          kc.x_ptrs, kc.n_windows, kc.Tk, kc.row_window.data_ptr(), kc.logits.data_ptr(),
                                                          kc.ws.data_ptr(), kc.ws.numel(), ops.stream_ptr()), "hirest_whisper_decode_step")
        kc.length += 1
        return kc.logits

    def step_rows(self, ctl: torch.Tensor, ids: torch.Tensor, kc: KVCache, stream=None) -> torch.Tensor:
        """one position for every row of a per-row cache that its record ``ctl [R, 8]`` has at a position (a row at -1 is left alone):
        ``ids`` int32 ``[R]`` on the device -> ``kc.logits [R, vocab_padded]``; on ``stream`` (a raw handle) or the current one"""
        _lib.check(_lib.load().hirest_whisper_decode_step_rows(C.byref(self._w()["desc"]), kc.R, ctl.data_ptr(), ids.data_ptr(), kc.k_ptrs, kc.v_ptrs,
                                                               kc.T_max, kc.x_ptrs, kc.n_windows, kc.Tk, kc.row_window.data_ptr(),
                                                               kc.logits.data_ptr(), kc.ws.data_ptr(), kc.ws.numel(),
                                                               ops.stream_ptr() if stream is None else stream), "hirest_whisper_decode_step_rows")
        return kc.logits


# ---------------------------------------------------------------------------------------------------------------------------------
# the tokenizer
# ---------------------------------------------------------------------------------------------------------------------------------

# whisper/tokenizer.py's tables: language code -> name in the order of the language tokens, and name or alias -> code
LANGUAGES = {
    "en": "english", "zh": "chinese", "de": "german", "es": "spanish", "ru": "russian", "ko": "korean", "fr": "french", "ja": "japanese",
    "pt": "portuguese", "tr": "turkish", "pl": "polish", "ca": "catalan", "nl": "dutch", "ar": "arabic", "sv": "swedish", "it": "italian",
    "id": "indonesian", "hi": "hindi", "fi": "finnish", "vi": "vietnamese", "he": "hebrew", "uk": "ukrainian", "el": "greek", "ms": "malay",
    "cs": "czech", "ro": "romanian", "da": "danish", "hu": "hungarian", "ta": "tamil", "no": "norwegian", "th": "thai", "ur": "urdu",
    "hr": "croatian", "bg": "bulgarian", "lt": "lithuanian", "la": "latin", "mi": "maori", "ml": "malayalam", "cy": "welsh", "sk": "slovak",
    "te": "telugu", "fa": "persian", "lv": "latvian", "bn": "bengali", "sr": "serbian", "az": "azerbaijani", "sl": "slovenian",
    "kn": "kannada", "et": "estonian", "mk": "macedonian", "br": "breton", "eu": "basque", "is": "icelandic", "hy": "armenian",
    "ne": "nepali", "mn": "mongolian", "bs": "bosnian", "kk": "kazakh", "sq": "albanian", "sw": "swahili", "gl": "galician",
    "mr": "marathi", "pa": "punjabi", "si": "sinhala", "km": "khmer", "sn": "shona", "yo": "yoruba", "so": "somali", "af": "afrikaans",
    "oc": "occitan", "ka": "georgian", "be": "belarusian", "tg": "tajik", "sd": "sindhi", "gu": "gujarati", "am": "amharic",
    "yi": "yiddish", "lo": "lao", "uz": "uzbek", "fo": "faroese", "ht": "haitian creole", "ps": "pashto", "tk": "turkmen", "nn": "nynorsk",
    "mt": "maltese", "sa": "sanskrit", "lb": "luxembourgish", "my": "myanmar", "bo": "tibetan", "tl": "tagalog", "mg": "malagasy",
    "as": "assamese", "tt": "tatar", "haw": "hawaiian", "ln": "lingala", "ha": "hausa", "ba": "bashkir", "jw": "javanese",
    "su": "sundanese", "yue": "cantonese"}
TO_LANGUAGE_CODE = {
    **{name: code for code, name in LANGUAGES.items()},
    "burmese": "my", "valencian": "ca", "flemish": "nl", "haitian": "ht", "letzeburgesch": "lb", "pushto": "ps", "panjabi": "pa",
    "moldavian": "ro", "moldovan": "ro", "sinhalese": "si", "castilian": "es", "mandarin": "zh"}
_LANGUAGE_TOKEN = re.compile(r"<\|([a-z]{2,3})\|>")
_UNICODE_SPLIT_LANGUAGES = frozenset(("zh", "ja", "th", "lo", "my", "yue"))      # written without spaces: words are unicode pieces


def language_code(language: str) -> str:
    """A language code, name or alias in any letter case ("de", "German", "castilian", "EN") -> its code; ValueError naming the value
    for anything else."""
    if isinstance(language, str):
        key = language.strip().lower()
        if key in LANGUAGES:
            return key
        if key in TO_LANGUAGE_CODE:
            return TO_LANGUAGE_CODE[key]
    raise ValueError(f"unsupported language: {language!r}")


class Tokenizer:
    """Whisper's tokenizer over the project's byte-level BPE (``bytebpe.ByteBPETokenizer``): GPT-2's vocabulary and merges plus
    Whisper's special tokens; the 1501 timestamp tokens ``<|0.00|>`` .. ``<|30.00|>`` follow ``<|notimestamps|>``.

    ``specials``: special-token string -> id.  ``<|endoftext|>``, ``<|startoftranscript|>``, ``<|startofprev|>`` and
    ``<|notimestamps|>`` are required; ``<|nospeech|>`` (``<|nocaptions|>`` in older files), ``<|startoflm|>``, ``<|transcribe|>``,
    ``<|translate|>`` and the language tokens (``<|en|>`` ...) are used when present."""

    def __init__(self, vocab: Dict[str, int], merges, specials: Dict[str, int], language: Optional[str] = None, task: Optional[str] = None):
        self.specials = {str(k): int(v) for k, v in specials.items()}
        for need in ("<|endoftext|>", "<|startoftranscript|>", "<|startofprev|>", "<|notimestamps|>"):
            if need not in self.specials:
                raise ValueError(f"the special-token table has no {need}")
        full = dict(vocab)
        full.update(self.specials)
        self.bpe = ByteBPETokenizer(full, merges, bos_token="<|endoftext|>", eos_token="<|endoftext|>", pad_token="<|endoftext|>",
                                    unk_token="<|no unknown token|>")     # every byte has a symbol in a real vocabulary
        self._special_ids = {i: s for s, i in self.specials.items()}
        self.language, self.task = language, task
        self.eot = self.specials["<|endoftext|>"]
        self.sot = self.specials["<|startoftranscript|>"]
        self.sot_prev = self.specials["<|startofprev|>"]
        self.sot_lm = self.specials.get("<|startoflm|>")
        self.no_speech = self.specials.get("<|nospeech|>", self.specials.get("<|nocaptions|>"))
        self.no_timestamps = self.specials["<|notimestamps|>"]
        self.transcribe, self.translate = self.specials.get("<|transcribe|>"), self.specials.get("<|translate|>")
        self.timestamp_begin = self.no_timestamps + 1

    @classmethod
    def from_dir(cls, model_dir: str, **kw) -> "Tokenizer":
        """A Hugging Face Whisper directory: ``vocab.json``, ``merges.txt`` and the added tokens (``added_tokens.json``, else the
        ``added_tokens`` of ``tokenizer.json``); ids of ``vocab.json`` that are special tokens are picked up from there."""
        with open(os.path.join(model_dir, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(model_dir, "merges.txt"), encoding="utf-8") as f:
            merges = f.read().split("\n")
        specials = {k: v for k, v in vocab.items() if k.startswith("<|") and k.endswith("|>")}
        added = os.path.join(model_dir, "added_tokens.json")
        if os.path.isfile(added):
            with open(added, encoding="utf-8") as f:
                specials.update(json.load(f))
        elif os.path.isfile(os.path.join(model_dir, "tokenizer.json")):
            with open(os.path.join(model_dir, "tokenizer.json"), encoding="utf-8") as f:
                specials.update({t["content"]: t["id"] for t in json.load(f).get("added_tokens", [])})
        specials = {k: v for k, v in specials.items() if not _TIMESTAMP.fullmatch(k)}
        return cls(vocab, merges, specials, **kw)

    @property
    def sot_sequence(self):
        seq = [self.sot]
        if self.language is not None:
            seq.append(self.specials[f"<|{self.language}|>"])
        if self.task is not None:
            seq.append(self.transcribe if self.task == "transcribe" else self.translate)
        return tuple(seq)

    @functools.cached_property
    def _language_table(self):
        """(ids ascending, their codes): the special tokens ``<|xx|>`` / ``<|xxx|>`` this vocabulary has whose code is a language —
        99 in the first multilingual vocabularies, 100 with ``yue``, none in an English-only one"""
        found = []
        for s, i in self.specials.items():
            m = _LANGUAGE_TOKEN.fullmatch(s)
            if m and m.group(1) in LANGUAGES:
                found.append((i, m.group(1)))
        found.sort()
        return tuple(i for i, _ in found), tuple(c for _, c in found)

    @property
    def all_language_tokens(self) -> Tuple[int, ...]:
        return self._language_table[0]

    @property
    def all_language_codes(self) -> Tuple[str, ...]:
        return self._language_table[1]

    @property
    def multilingual(self) -> bool:
        """Whether this tokenizer was set up as a multilingual checkpoint's: it has language tokens AND was given a language or a task.
        Which tokens exist does not decide it — the English-only vocabularies of the released ``*.en`` checkpoints carry ``<|en|>`` ..
        ``<|su|>`` as well — but how the tokenizer was configured, as in Whisper, whose ``get_tokenizer`` leaves language and task at
        None for an English-only model: ``load_model`` does the same, ``with_language(None, "transcribe")`` is multilingual with the
        language to be detected."""
        return bool(self.all_language_tokens) and (self.language is not None or self.task is not None)

    @property
    def language_token(self) -> int:
        """the id of ``<|language|>`` for this tokenizer's language (Whisper's ``language_token``)"""
        if self.language is None:
            raise ValueError("this tokenizer does not have a language configured")
        return self.to_language_token(self.language)

    def to_language_token(self, language: str) -> int:
        token = self.specials.get(f"<|{language}|>")
        if token is None or token not in self.all_language_tokens:
            raise KeyError(f"language {language!r} not found in the tokenizer")
        return token

    def with_language(self, language: Optional[str], task: Optional[str] = "transcribe") -> "Tokenizer":
        """Whisper's ``get_tokenizer(multilingual, language=, task=)`` from this one: a copy with that language (a code, name or alias;
        None: to be detected) and task (transcribe, as Whisper's default for a multilingual model, or translate) that shares the BPE
        and every table; this tokenizer is not changed.  ``with_language(None, None)`` is the English-only configuration."""
        if language is not None:
            language = language_code(language)
            if self.all_language_tokens and language not in self.all_language_codes:
                raise ValueError(f"unsupported language: {language!r} has no token in this vocabulary")
        if task not in (None, "transcribe", "translate"):
            raise ValueError(f"unsupported task: {task!r} (transcribe or translate)")
        other = copy.copy(self)
        other.language, other.task = language, task
        return other

    def encode(self, text: str) -> List[int]:
        return self.bpe.tokenize_ids(text)

    def _decode(self, ids, stamps: bool) -> str:
        out, run = [], []
        for t in ids:
            t = int(t)
            if t >= self.timestamp_begin or t in self._special_ids:
                if run:
                    out.append(self.bpe.decode(run))
                    run = []
                if t >= self.timestamp_begin:
                    if stamps:
                        out.append(f"<|{(t - self.timestamp_begin) * 0.02:.2f}|>")
                else:
                    out.append(self._special_ids[t])
            else:
                run.append(t)
        if run:
            out.append(self.bpe.decode(run))
        return "".join(out)

    def decode(self, ids) -> str:
        """text of the ids, timestamp tokens dropped (Whisper's ``decode``)"""
        return self._decode(ids, False)

    def decode_with_timestamps(self, ids) -> str:
        """timestamp tokens rendered as ``<|1.08|>`` (0.02 s per token)"""
        return self._decode(ids, True)

    def split_to_word_tokens(self, tokens):
        """Whisper's ``split_to_word_tokens``: ``(words, word_tokens)``.  zh, ja, th, lo, my and yue split on unicode boundaries, every
        other language (and no language) on spaces."""
        if self.language in _UNICODE_SPLIT_LANGUAGES:
            return self.split_tokens_on_unicode(tokens)
        return self.split_tokens_on_spaces(tokens)

    def split_tokens_on_unicode(self, tokens):
        """a piece ends where the tokens so far decode to complete characters (no U+FFFD that the whole text does not have there)"""
        full = self.decode_with_timestamps(tokens)
        words, word_tokens, current, offset = [], [], [], 0
        for token in tokens:
            current.append(int(token))
            decoded = self.decode_with_timestamps(current)
            if "\ufffd" not in decoded or full[offset + decoded.index("\ufffd")] == "\ufffd":
                words.append(decoded)
                word_tokens.append(current)
                current = []
                offset += len(decoded)
        return words, word_tokens

    def split_tokens_on_spaces(self, tokens):
        """the unicode pieces joined into words: a new word starts at a piece that starts with a space, is punctuation alone, or is a
        special token"""
        words, word_tokens = [], []
        for piece, piece_tokens in zip(*self.split_tokens_on_unicode(tokens)):
            special = piece_tokens[0] >= self.eot
            if special or piece.startswith(" ") or piece.strip() in string.punctuation or not words:
                words.append(piece)
                word_tokens.append(piece_tokens)
            else:
                words[-1] += piece
                word_tokens[-1].extend(piece_tokens)
        return words, word_tokens

    @functools.cached_property
    def non_speech_tokens(self):
        """What ``suppress_tokens="-1"`` stands for: tokens of speaker tags and non-speech annotations (``♪♪♪``, ``( SPEAKING FOREIGN
        LANGUAGE )``, ``[DAVID] Hey there``) — the listed symbols where they are one token, with and without a leading space; of the
        musical symbols the first token even where they take several; `` -`` and `` '`` so that they do not open a line."""
        symbols = list("\"#()*+/:;<=>@[\\]^_`{|}~「」『』")
        symbols += "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split()
        misc = set("♩♪♫♬♭♮♯")
        result = {self.encode(" -")[0], self.encode(" '")[0]}
        for sym in symbols + sorted(misc):
            for text in (sym, " " + sym):
                try:
                    toks = self.encode(text)
                except KeyError:                                      # a reduced vocabulary without that byte: nothing to suppress
                    continue
                if len(toks) == 1 or sym in misc:
                    result.add(toks[0])
        return tuple(sorted(result))


# ---------------------------------------------------------------------------------------------------------------------------------
# decoding
# ---------------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class DecodingOptions:
    task: str = "transcribe"                  # or "translate"; "transcribe" yields to a tokenizer made with with_language(.., "translate")
    language: Optional[str] = None            # a code, name or alias; None: the tokenizer's, else detected (multilingual tokenizers only)
    temperature: float = 0.0
    sample_len: Optional[int] = None          # maximum number of tokens to sample (default: half the text context)
    best_of: Optional[int] = None             # independent candidates when temperature > 0
    beam_size: Optional[int] = None           # not built: beam search
    patience: Optional[float] = None          # not built: beam search
    length_penalty: Optional[float] = None    # None: rank candidates by sum_logprobs / length
    prompt: Optional[Union[str, List[int]]] = None
    prefix: Optional[Union[str, List[int]]] = None      # not built
    suppress_blank: bool = True
    suppress_tokens: Optional[Union[str, Iterable[int]]] = "-1"
    without_timestamps: bool = False
    max_initial_timestamp: Optional[float] = 1.0
    fp16: bool = True                         # accepted and ignored: the decoder is exact fp32; the encoder's precision is the model's
                                              # (Whisper.set_precision / load_model(precision=) / HIREST_WHISPER_PRECISION)
    seed: int = 0                             # of the counter-based generator the categorical draws come from (not Whisper's: it draws from torch's)
    monotonic_timestamps: bool = True         # current Whisper's rule that timestamps do not decrease

    def __post_init__(self):
        if self.beam_size is not None or self.patience is not None:
            raise NotImplementedError("beam search (beam_size / patience) is not built: the sampling branch (temperature, best_of) is")
        if self.prefix is not None:
            raise NotImplementedError("prefix is not built")
        if self.length_penalty is not None:
            raise NotImplementedError("length_penalty other than None is not built")
        if self.temperature == 0 and self.best_of is not None:
            raise ValueError("best_of with greedy sampling (T=0) is not compatible")


@dataclasses.dataclass(frozen=True)
class DecodingResult:
    audio_features: Optional[torch.Tensor] = None
    language: str = "en"
    tokens: List[int] = dataclasses.field(default_factory=list)
    text: str = ""
    avg_logprob: float = float("nan")
    no_speech_prob: float = float("nan")
    temperature: float = float("nan")
    compression_ratio: float = float("nan")
    language_probs: Optional[Dict[str, float]] = None      # detect_language's, where decode() detected the window's language


def compression_ratio(text: str) -> float:
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def tail_params(tokenizer: Tokenizer, options: DecodingOptions, n_vocab: int, vocab_padded: int, n_audio_ctx: int, sample_begin: int,
                device) -> Tuple["_lib.WhisperTailParams", torch.Tensor]:
    """The tail kernel's constant block for a tokenizer and options, and the suppress mask it points to (keep it alive)."""
    sup = options.suppress_tokens
    if isinstance(sup, str):
        sup = [int(t) for t in sup.split(",") if t.strip()]
    sup = list(sup or [])
    if -1 in sup:
        sup = [t for t in sup if t >= 0] + list(tokenizer.non_speech_tokens)
    sup += [t for t in (tokenizer.transcribe, tokenizer.translate, tokenizer.sot, tokenizer.sot_prev, tokenizer.sot_lm, tokenizer.no_speech)
            if t is not None]
    sup += list(range(n_vocab, vocab_padded))                         # the LM head's pad columns
    words = np.zeros((vocab_padded + 31) // 32, dtype=np.uint32)
    for t in set(sup):
        if not 0 <= t < vocab_padded:
            raise ValueError(f"suppressed token {t} outside the vocabulary of {n_vocab}")
        words[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    mask = torch.from_numpy(words.view(np.int32)).to(device)
    blank = tokenizer.encode(" ")
    p = _lib.WhisperTailParams()
    p.n_vocab, p.eot, p.no_speech = n_vocab, tokenizer.eot, -1 if tokenizer.no_speech is None else tokenizer.no_speech
    p.no_timestamps, p.timestamp_begin = tokenizer.no_timestamps, tokenizer.timestamp_begin
    p.max_initial_timestamp_index = -1
    if options.max_initial_timestamp is not None:
        p.max_initial_timestamp_index = int(round(options.max_initial_timestamp / (CHUNK_LENGTH / n_audio_ctx)))
    p.sample_begin, p.blank, p.suppress_blank = sample_begin, blank[0] if len(blank) == 1 else -1, int(bool(options.suppress_blank))
    p.timestamp_rules, p.monotonic = int(not options.without_timestamps), int(bool(options.monotonic_timestamps))
    p.temperature, p.seed, p.serial = float(options.temperature), int(options.seed) & 0xFFFFFFFF, 0
    p.suppress_mask = mask.data_ptr()
    return p, mask


def new_row_state(R: int, device) -> torch.Tensor:
    """``hirest_whisper_row_state [R]`` as an int32 ``[R, 8]`` tensor in its initial state (columns 5 .. 7 are floats)"""
    st = torch.zeros((R, _lib.WHISPER_ROW_STATE_WORDS), dtype=torch.int32)
    st[:, 1:4] = -1
    return st.to(device)


def _prompt_language(tokenizer: Tokenizer, options: DecodingOptions) -> Optional[str]:
    """The code of the language a window's prompt names on a multilingual tokenizer: ``options.language`` (a code, name or
    alias) when given, else the tokenizer's own; None: neither names one, and ``decode`` detects it."""
    if options.language is not None:
        return language_code(options.language)
    return tokenizer.language


def _initial_tokens(tokenizer: Tokenizer, options: DecodingOptions, n_ctx: int, language: Optional[str] = None) -> Tuple[List[int], int]:
    """(a window's initial tokens, the index of ``<|startoftranscript|>`` among them).  A multilingual tokenizer (``Tokenizer.
    multilingual``) gets Whisper's ``sot, <|language|>, <|task|>``: the language is ``language`` (what ``decode`` detected) or
    ``_prompt_language``'s, the task is ``options.task`` and, where that is left at "transcribe", the task the tokenizer was given
    (``with_language(.., "translate")``) — so ``DecodingOptions(task="transcribe")`` cannot ask a tokenizer made for translation to
    transcribe: give the model ``tokenizer.with_language(language, "transcribe")`` instead.  An English-only tokenizer ignores both
    options, whatever tokens its vocabulary has, and the prompt starts with its own ``sot_sequence``."""
    if tokenizer.multilingual:
        language = language or _prompt_language(tokenizer, options)
        if language is None:
            raise ValueError("no language: neither options.language nor the tokenizer names one (decode() detects it before it builds the prompt)")
        task = options.task if options.task != "transcribe" else tokenizer.task or "transcribe"
        if task not in ("transcribe", "translate"):
            raise NotImplementedError(f"task {task!r} is not built: transcribe or translate")
        task_token = tokenizer.transcribe if task == "transcribe" else tokenizer.translate
        if task_token is None:
            raise ValueError(f"the special-token table has no <|{task}|>")
        try:
            tokens = [tokenizer.sot, tokenizer.to_language_token(language), task_token]
        except KeyError as e:
            raise ValueError(f"unsupported language: {language!r} has no token in this vocabulary") from e
    else:
        tokens = list(tokenizer.sot_sequence)
    if options.without_timestamps:
        tokens.append(tokenizer.no_timestamps)
    if options.prompt:                                                # (an empty prompt — a file's first window — adds no sot_prev either)
        prompt = tokenizer.encode(" " + options.prompt.strip()) if isinstance(options.prompt, str) else list(options.prompt)
        tokens = [tokenizer.sot_prev] + prompt[-(n_ctx // 2 - 1):] + tokens
    return tokens, tokens.index(tokenizer.sot)


_PER_WINDOW_OPTIONS = ("prompt", "temperature", "best_of", "seed", "language")     # what may differ between the windows of one decode_many call
_ROWS_PER_CALL = 256           # hirest_gemm_f32_ln's forms, which the step's LayerNorm GEMMs rely on, take up to 256 rows
FILES_IN_FLIGHT = 16           # transcribe_many's default: the largest of the sweep in DESIGN §4.17, where windows/s was still growing


def new_row_ctl(rows, device) -> torch.Tensor:
    """``hirest_whisper_row_ctl [R]`` as an int32 ``[R, 8]`` tensor from ``(position, step, max_steps, draw_row, seed, temperature)`` per row"""
    ctl = np.zeros((len(rows), _lib.WHISPER_ROW_CTL_WORDS), dtype=np.int32)
    for r, (position, step, max_steps, draw_row, seed, temperature) in enumerate(rows):
        ctl[r, :4] = position, step, max_steps, draw_row
        ctl[r, 4:5].view(np.uint32)[0] = int(seed) & 0xFFFFFFFF
        ctl[r, 5:6].view(np.float32)[0] = float(temperature)
    return torch.from_numpy(ctl).to(device)


def _audio_states(model, mel: torch.Tensor) -> torch.Tensor:
    """windows ``[W, n_mels, 3000]`` through the encoder, in one call — or, already encoder states ``[W, Tk, D]``, as they are"""
    if mel.shape[-2:] == (model.dims["n_audio_ctx"], model.dims["n_audio_state"]):
        return mel.to(model.device, torch.float32)
    return model.encoder(mel)


@torch.no_grad()
def detect_language(model: "Whisper", mel: torch.Tensor, tokenizer: Optional[Tokenizer] = None):
    """``whisper.detect_language``: one window ``[n_mels, 3000]`` (or its encoder states ``[Tk, D]``) or a batch of W of them ->
    ``(language_tokens, language_probs)``: the id of the most probable language token per window (an int64 tensor ``[W]`` on the host)
    and per window a dict code -> probability over the tokenizer's languages (the softmax of the ``<|startoftranscript|>`` position's
    logits over the language tokens alone); a tensor without dimensions and one dict for a single window.  ValueError when the
    tokenizer is not multilingual (``Tokenizer.multilingual``: no language tokens, or an English-only checkpoint's configuration).

    One encoder call and one cross key / value projection for all windows, ONE pass of ``<|startoftranscript|>`` at position 0 through
    the per-row decode step with row w attending window w (a cache of one position), ``hirest_whisper_language_tail`` on its logits,
    and one read-back.  A window's values do not depend on the others of the call."""
    tokenizer = tokenizer if tokenizer is not None else getattr(model, "tokenizer", None)
    if tokenizer is None:
        raise ValueError("the model has no tokenizer: load_model(path, tokenizer=...) or detect_language(..., tokenizer=...)")
    table, codes = tokenizer.all_language_tokens, tokenizer.all_language_codes
    if not tokenizer.multilingual:                                    # (Whisper's check, too, is of how the tokenizer was configured)
        raise ValueError("this model doesn't have language tokens so it can't perform lang id: the tokenizer has none, or is English-only's")
    L = len(table)
    single = mel.ndim == 2
    if single:
        mel = mel[None]
    dec, dev, lib = model.decoder, model.device, _lib.load()
    if L > 128 or table[-1] >= dec.vocab:
        raise ValueError(f"{L} language tokens up to id {table[-1]}: at most 128, inside the vocabulary of {dec.vocab}")
    with torch.cuda.device(dev):
        xa = _audio_states(model, mel)
        W = int(xa.shape[0])
        ids_table = torch.tensor(table, dtype=torch.int32, device=dev)
        found = torch.empty((W,), dtype=torch.int32, device=dev)
        probs = torch.empty((W, L), dtype=torch.float32, device=dev)
        for r0 in range(0, W, _ROWS_PER_CALL):
            R = min(_ROWS_PER_CALL, W - r0)
            kc = KVCache(dec, xa[r0:r0 + R], torch.arange(R, dtype=torch.int32), 1, per_row=True)
            ctl = new_row_ctl([(0, 0, 1, 0, 0, 0.0)] * R, dev)                   # every row at position 0
            ids = torch.full((R,), tokenizer.sot, dtype=torch.int32, device=dev)
            dec.step_rows(ctl, ids, kc)
            _lib.check(lib.hirest_whisper_language_tail(kc.logits.data_ptr(), dec.vocab_padded, R, dec.vocab, ids_table.data_ptr(), L,
                                                        found[r0:].data_ptr(), probs[r0:].data_ptr(), ops.stream_ptr()),
                       "hirest_whisper_language_tail")
        tokens, rows = found.cpu().to(torch.int64), probs.cpu().tolist()          # the call's only read-back, after every pass is enqueued
    dicts = [dict(zip(codes, row)) for row in rows]
    return (tokens[0], dicts[0]) if single else (tokens, dicts)


@torch.no_grad()
def decode(model: "Whisper", mel: torch.Tensor, options: DecodingOptions = DecodingOptions(), *, return_candidates: bool = False,
           graph: Optional[bool] = None):
    """``whisper.decode``: one 30-second window ``[n_mels, 3000]`` (or encoder states ``[Tk, D]``) or a batch of them -> a
    ``DecodingResult`` (a list for a batch).  Greedy at temperature 0; at temperature > 0 ``best_of`` candidates per window are sampled
    and the one with the highest ``sum_logprobs / length`` is returned.  A window is one run of the decoding loop (``_decode_rows``) over
    its candidate rows.  A batch runs one loop per window, in order; whoever wants the windows in one loop calls ``decode_many()``.
    With a multilingual tokenizer (``Tokenizer.multilingual``: what ``load_model`` gives a multilingual checkpoint) the prompt names
    ``options.language`` (else the tokenizer's language) and ``options.task`` (transcribe or translate; left at "transcribe" it
    yields to the task the tokenizer was made with, so a ``with_language(.., "translate")`` tokenizer translates whatever
    ``options.task`` says — see ``_initial_tokens``); an English-only one ignores both.  Where neither names a language, the windows' languages are detected first, in one ``detect_language``
    pass, and ``result.language`` / ``result.language_probs`` say what was found.  ``task="lang_id"`` is not built: call
    ``detect_language``.  ``return_candidates``: also every candidate's (tokens, sum_logprobs) per window (tests).  ``graph``: replay the
    loop's iterations from a captured hipGraph (``None``: the environment's ``HIREST_WHISPER_GRAPH``, else off) — the same
    values bit for bit, fewer launches on the host."""
    single = mel.ndim == 2
    if single:
        mel = mel[None]
    results, everything = _decode_windows(model, mel, [options] * int(mel.shape[0]), 0,         # 0 rows fit beside a window: one per loop
                                          **({"graph": True} if resolve_graph(graph) else {}))
    if return_candidates:
        return (results[0], everything[0]) if single else (results, everything)
    return results[0] if single else results


@torch.no_grad()
def decode_many(model: "Whisper", mels, options: Union[DecodingOptions, Sequence[DecodingOptions]] = DecodingOptions(), *,
                return_candidates: bool = False, graph: Optional[bool] = None):
    """``decode`` for W windows that need not share their options — the current windows of W files — in ONE run of the decoding loop:
    ``mels`` W spectrograms ``[n_mels, 3000]`` or encoder states ``[Tk, D]`` (a tensor or a sequence of them), ``options`` one
    ``DecodingOptions`` or W of them.  ``prompt``, ``temperature``, ``best_of``, ``seed`` and ``language`` may differ between windows; any other field
    that does raises ValueError.  Returns a list of W ``DecodingResult`` with the values ``decode`` gives window by window, bit for bit
    (the same loop, whose rows do not depend on their neighbours); ``return_candidates`` as ``decode``'s.  More than 256 candidate rows
    are split into consecutive loops.  ``graph`` as ``decode``'s."""
    mel = mels if torch.is_tensor(mels) else torch.stack([m.to(model.device) for m in mels])
    if mel.ndim != 3:
        raise ValueError(f"decode_many takes W windows [W, n_mels, frames] or [W, Tk, D], not a tensor of shape {tuple(mel.shape)}")
    W = int(mel.shape[0])
    opts = [options] * W if isinstance(options, DecodingOptions) else list(options)
    if len(opts) != W:
        raise ValueError(f"{len(opts)} DecodingOptions for {W} windows")
    for f in dataclasses.fields(DecodingOptions):
        if f.name not in _PER_WINDOW_OPTIONS and any(getattr(o, f.name) != getattr(opts[0], f.name) for o in opts):
            raise ValueError(f"decode_many: {f.name} differs between the windows of one call (only {', '.join(_PER_WINDOW_OPTIONS)} may)")
    results, everything = _decode_windows(model, mel, opts, _ROWS_PER_CALL, **({"graph": True} if resolve_graph(graph) else {}))
    return (results, everything) if return_candidates else results


def _decode_windows(model, mel, opts, rows_per_loop, graph=False):
    """What ``decode`` and ``decode_many`` share: the plan of every window (initial tokens, sot index, step budget cut by the context,
    candidate rows), one encoder call for all of them, and consecutive windows — as many as fit ``rows_per_loop`` candidate rows, at
    least one — through ``_decode_rows``.  -> (results, candidates), one entry per window."""
    tokenizer, dec, dev = model.tokenizer, model.decoder, model.device
    if graph:
        dec._require_gpu()                                            # (before anything of the option is looked at: no CPU form of it either)
    if tokenizer is None:
        raise ValueError("the model has no tokenizer: load_model(path, tokenizer=...) or set model.tokenizer")
    codes = tokenizer.all_language_codes if tokenizer.multilingual else ()
    # per window (language code, detect_language's probabilities): (None, None) on an English-only tokenizer
    langs = [(_prompt_language(tokenizer, o) if codes else None, None) for o in opts]
    detect = [w for w, (code, _) in enumerate(langs) if codes and code is None]
    plans = []
    for o, (code, _) in zip(opts, langs):
        # (a window whose language is still to be detected is planned with a stand-in: the prompt's length does not depend on it)
        initial, sot_index = _initial_tokens(tokenizer, o, dec.ctx, code or (codes[0] if codes else None))
        steps = min(dec.ctx, len(initial) + (o.sample_len or dec.ctx // 2)) - len(initial)
        if steps <= 0:
            raise ValueError(f"a prompt of {len(initial)} tokens leaves no room to sample in a context of {dec.ctx}")
        plans.append((initial, sot_index, steps, (o.best_of or 1) if o.temperature > 0 else 1))
    results, everything = [], []
    with torch.cuda.device(dev):
        xa = _audio_states(model, mel)
        if detect:                                                    # all of the call's undetermined windows in one pass, before any prefill
            found, probs = detect_language(model, xa[detect], tokenizer)
            for w, token, p in zip(detect, found.tolist(), probs):
                langs[w] = (codes[tokenizer.all_language_tokens.index(token)], p)
                plans[w][0][plans[w][1] + 1] = token
        w0 = 0
        while w0 < len(plans):
            w1, rows = w0 + 1, plans[w0][3]
            while w1 < len(plans) and rows + plans[w1][3] <= rows_per_loop:
                rows += plans[w1][3]
                w1 += 1
            res, cands = _decode_rows(model, xa[w0:w1], opts[w0:w1], plans[w0:w1], langs[w0:w1], graph)
            results += res
            everything += cands
            w0 = w1
    return results, everything


# The loop replayed from a hipGraph.  Every per-step quantity is on the device (the rows' records, and the call's number
# in the counted tail), so ONE captured run of DECODE_GRAPH_CHUNK x {tail, step} serves every token of every window whose loop has the
# arena's shape: the eager loop's ``DecodeState`` at the decoder's whole context, kept for its stable addresses under (device, stream,
# R, n_windows, Tk).  The loops differ in who issues the iterations (``_eager_loop`` / ``_replay_loop``) and in the tail's entry only.
DECODE_GRAPH_CHUNK = 8         # iterations per captured graph (as CAPTION_GRAPH_CHUNK; profiles/whisper_graph.txt has 4 and 16 beside it)
DECODE_ARENAS = 4              # arenas kept per decoder, least recently used first out


def resolve_graph(graph: Optional[bool]) -> bool:
    """The ``graph=`` keyword of ``decode`` / ``decode_many`` / ``transcribe`` / ``transcribe_many``: the keyword where it is given, else
    the environment's ``HIREST_WHISPER_GRAPH`` (set and not ``0``), else off.  Each of the four hands ``graph=True`` on where it is on
    and nothing where it is off (the calls of before, which the host tests' stand-ins take); ``_decode_windows`` hands on a plain bool."""
    if graph is not None:
        return bool(graph)
    return os.environ.get("HIREST_WHISPER_GRAPH", "").strip() not in ("", "0")


def graph_throttle(issued: int, stamp: int, chunk: int, max_steps: int) -> str:
    """What the replaying loop does next, a pure function of the chunks it has issued and the pinned stamp it has just read: ``"stop"``,
    ``"wait"`` (poll the stamp again) or ``"issue"`` (replay one more chunk).  The stamp is ``(tails landed << 1) | no row is active``;
    iteration 0 ran eagerly, so after ``issued`` chunks ``1 + issued * chunk`` tails are enqueued.  Stop when no row is active, when
    ``max_steps`` tails have landed, or when every tail a row can need is enqueued (the caller then synchronises).  Otherwise at most
    two chunks are in flight: the next is issued only once the chunk before the last has landed."""
    if issued < 0 or chunk < 1 or max_steps < 1 or stamp < 0:
        raise ValueError(f"graph_throttle({issued}, {stamp}, {chunk}, {max_steps})")
    landed = stamp >> 1
    if (stamp & 1) or landed >= max_steps or 1 + issued * chunk >= max_steps:
        return "stop"
    if issued >= 2 and landed < 1 + (issued - 1) * chunk:
        return "wait"
    return "issue"


def _decode_arena(decoder: "TextDecoder", R: int, n_windows: int, Tk: int) -> DecodeState:
    """The arena of (device, current stream, R, n_windows, Tk), made on first use: a ``DecodeState`` of the decoder's whole context
    per row and ``n_text_ctx // 2`` tokens.  The arenas live in the decoder's weight preparation — their graphs hold its addresses —
    so any move or cast drops them all; of more than ``DECODE_ARENAS`` the least recently used goes."""
    arenas = decoder._w().setdefault("decode_arenas", collections.OrderedDict())
    dev = decoder.device
    with torch.cuda.device(dev):
        key = (dev.index, ops.stream_ptr(), R, n_windows, Tk)
        if key not in arenas:
            while len(arenas) >= DECODE_ARENAS:
                arenas.popitem(last=False)
            arenas[key] = DecodeState(decoder, R, n_windows, Tk, decoder.ctx, decoder.ctx // 2)
    arenas.move_to_end(key)
    return arenas[key]


def _eager_loop(dec: "TextDecoder", kc: DecodeState, params, max_steps: int) -> None:
    """The loop's iterations launch by launch: tail, then step, until the pinned stamp says that no row is active; no step after the last tail."""
    for call in range(max_steps):
        dec.graph_stats["eager_steps"] += 1
        kc.tail(params, call)
        if (int(kc.stamp_host[0]) & 1) or call == max_steps - 1:      # whatever call has landed by now: no wait
            break
        dec.step_rows(kc.ctl, kc.ids, kc)


def _replay_loop(dec: "TextDecoder", kc: DecodeState, params, max_steps: int) -> None:
    """The same iterations on an arena: iteration 0 eagerly (also the warm-up of a capture), then the captured chunk of
    ``DECODE_GRAPH_CHUNK`` x {counted tail, step} replayed as ``graph_throttle`` says.  The only thing the host reads is the pinned
    stamp; nothing here synchronises with the device but a capture."""
    stats = dec.graph_stats

    def iteration(stream):
        kc.tail(params, stream=stream)
        dec.step_rows(kc.ctl, kc.ids, kc, stream)
    # what a capture bakes in beside the arena's addresses: the tail's constants (not the four fields the rows' records replace)
    baked = type(params).from_buffer_copy(params)
    baked.temperature, baked.seed, baked.serial, baked.sample_begin = 0.0, 0, 0, 0
    key = (bytes(baked), int(kc.tokens.shape[1]), max(1, int(DECODE_GRAPH_CHUNK)))
    kc.count.zero_()
    iteration(ops.stream_ptr())
    stats["eager_steps"] += 1
    chunk = key[2]
    issued, stream, polls = 0, torch.cuda.current_stream(), 0
    while True:
        seen = int(kc.stamp_host[0])
        act = graph_throttle(issued, seen, chunk, max_steps)
        if act == "stop":
            return
        if act == "wait":
            polls += 1
            if polls % 4096 == 0 and stream.query() and int(kc.stamp_host[0]) == seen:      # an idle stream and no new stamp: no tail will land
                raise RuntimeError(f"{_NAME}: the replayed decoding loop stopped at stamp {seen} with {issued} chunks issued")
            continue
        if kc.graph is None or kc.graph_key != key:
            kc.graph = kc.graph_key = None
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st = ops.stream_ptr()
                for _ in range(chunk):
                    iteration(st)
            kc.graph, kc.graph_key = g, key
            stats["captures"] += 1
        kc.graph.replay()
        stats["replays"] += 1
        issued, polls = issued + 1, 0


def _decode_rows(model, xa, opts, plans, langs, graph: bool = False):
    """THE decoding loop, over the candidate rows of ``xa``'s windows: one ``DecodeState`` for all rows, one cross key / value
    projection for all windows into it (``load``), one ragged prefill of all windows' prompts (``prefill_many``), the rows' records
    and first logits (``reset``), then per token a tail (``DecodeState.tail``) and a step (``TextDecoder.step_rows``) over all rows —
    each at its own position, with its own temperature, seed and remaining room, kept in a device record per row — until no row is
    active.  Nothing is read back in the loop but the pinned stamp; tokens and sums are read once at the end.
    ``graph`` chooses the state and who issues the iterations, nothing else: off, a state sized for this loop and ``_eager_loop``; on,
    the arena of the loop's shape and ``_replay_loop``, which replays the iterations after the first — the same bits."""
    tokenizer, dec, dev, lib = model.tokenizer, model.decoder, model.device, _lib.load()
    Vp = dec.vocab_padded
    first_row = np.cumsum([0] + [p[3] for p in plans]).tolist()
    R = first_row[-1]
    max_steps = max(steps for _, _, steps, _ in plans)
    row_window = torch.tensor([w for w, p in enumerate(plans) for _ in range(p[3])], dtype=torch.int32)
    if graph:
        if max_steps > dec.ctx // 2:
            raise ValueError(f"graph=True: {max_steps} steps to sample, the arena's tokens hold n_text_ctx // 2 = {dec.ctx // 2}")
        kc, run = _decode_arena(dec, R, int(xa.shape[0]), int(xa.shape[1])), _replay_loop
    else:
        T_max = max(len(initial) + steps for initial, _, steps, _ in plans)
        kc, run = DecodeState(dec, R, int(xa.shape[0]), int(xa.shape[1]), T_max, max_steps), _eager_loop
    kc.load(dec, xa, row_window)
    # the constants every window shares; temperature, seed, serial and sample_begin are the rows' own (hirest_whisper_row_ctl)
    params, mask = tail_params(tokenizer, opts[0], dec.vocab, Vp, model.dims["n_audio_ctx"], 0, "cpu")
    kc.mask.copy_(mask)
    params.suppress_mask = kc.mask.data_ptr()
    # every window's prompt in one ragged pass: the caches, the logits of the last position and, where it is another one, of sot's
    groups = [p[3] for p in plans]
    want_sot = tokenizer.no_speech is not None
    last, at_sot = dec.prefill_many([p[0] for p in plans], kc, first_row[:-1], groups, range(len(plans)),
                                    [p[1] for p in plans] if want_sot else None)
    no_speech, ctl_rows = [], []
    for w, (initial, sot_index, steps, group) in enumerate(plans):
        T = len(initial)
        scratch = None
        if sot_index != T - 1 and want_sot:
            # Whisper reads no_speech_prob at the sot position: one lock-step tail call on that row, into a scratch state
            scratch, sid = new_row_state(1, dev), torch.empty(1, dtype=torch.int32, device=dev)
            _lib.check(lib.hirest_whisper_step_tail(at_sot[w].data_ptr(), Vp, 1, Vp, 0, 0, C.byref(params), scratch.data_ptr(), sid.data_ptr(), None,
                                                    None, None, ops.stream_ptr()), "hirest_whisper_step_tail")
        no_speech.append(scratch)
        ctl_rows += [(T - 1, 0, steps, g, opts[w].seed, opts[w].temperature) for g in range(group)]
    kc.reset(ctl_rows, tokenizer.eot, last)
    run(dec, kc, params, max_steps)
    torch.cuda.current_stream().synchronize()
    toks, st = kc.tokens.cpu().numpy(), kc.state.cpu()
    sums = st[:, 5].view(torch.float32).tolist()
    results, everything = [], []
    for w, (initial, sot_index, steps, group) in enumerate(plans):
        r0 = first_row[w]
        nsp = (no_speech[w].cpu()[0] if no_speech[w] is not None else st[r0])[6:7].view(torch.float32).item()
        cands = []
        for g in range(group):
            row = toks[r0 + g, :steps].tolist()
            cands.append((row[:row.index(tokenizer.eot)] if tokenizer.eot in row else row, sums[r0 + g]))
        best = max(range(group), key=lambda g: (cands[g][1] / max(len(cands[g][0]), 1), -g))
        t, lp = cands[best]
        text = tokenizer.decode(t).strip()
        results.append(DecodingResult(audio_features=xa[w], language=langs[w][0] or tokenizer.language or "en", tokens=t, text=text,
                                      avg_logprob=lp / (len(t) + 1), no_speech_prob=nsp, temperature=opts[w].temperature,
                                      compression_ratio=compression_ratio(text) if text else 0.0, language_probs=langs[w][1]))
        everything.append(cands)
    return results, everything


# ---------------------------------------------------------------------------------------------------------------------------------
# the model, transcribe(), .srt
# ---------------------------------------------------------------------------------------------------------------------------------

class Whisper(nn.Module):
    """``whisper.model.Whisper``: ``.encoder``, ``.decoder``, ``.dims`` (OpenAI's field names), ``embed_audio``, ``logits``, ``forward``."""

    def __init__(self, dims_or_config, state_dict: Dict[str, torch.Tensor], tokenizer: Optional[Tokenizer] = None):
        super().__init__()
        self.encoder = AudioEncoder(dims_or_config, state_dict)
        self.decoder = TextDecoder(dims_or_config, state_dict)
        e, d = self.encoder, self.decoder
        self.dims = {"n_mels": e.n_mels, "n_audio_ctx": e.ctx, "n_audio_state": e.width, "n_audio_head": e.heads, "n_audio_layer": e.layers,
                     "n_vocab": d.vocab, "n_text_ctx": d.ctx, "n_text_state": d.width, "n_text_head": d.heads, "n_text_layer": d.layers}
        self.tokenizer = tokenizer
        # The heads whose cross-attention the word alignment reads (``find_alignment``): every head of the last half of the layers,
        # Whisper's own default.  The released checkpoints' tuned lists are not shipped: ``set_alignment_heads`` takes them.
        self.alignment_heads = torch.zeros((d.layers, d.heads), dtype=torch.bool)
        self.alignment_heads[d.layers // 2:] = True

    def set_alignment_heads(self, mask_or_pairs) -> None:
        """Replace ``alignment_heads``: a bool mask ``[layers, heads]`` or a sequence of (layer, head) pairs"""
        d = self.decoder
        if torch.is_tensor(mask_or_pairs) and mask_or_pairs.dtype == torch.bool or isinstance(mask_or_pairs, np.ndarray) and mask_or_pairs.dtype == bool:
            mask = torch.as_tensor(mask_or_pairs).cpu().clone()
            if tuple(mask.shape) != (d.layers, d.heads):
                raise ValueError(f"a mask of shape {tuple(mask.shape)}: [{d.layers}, {d.heads}] expected")
        else:
            mask = torch.zeros((d.layers, d.heads), dtype=torch.bool)
            for layer, head in mask_or_pairs:
                if not (0 <= int(layer) < d.layers and 0 <= int(head) < d.heads):
                    raise ValueError(f"(layer {layer}, head {head}): the decoder has {d.layers} layers of {d.heads} heads")
                mask[int(layer), int(head)] = True
        if not bool(mask.any()):
            raise ValueError("no alignment head selected")
        self.alignment_heads = mask

    @property
    def device(self) -> torch.device:
        return self.decoder.device

    @property
    def is_multilingual(self) -> bool:
        return self.dims["n_vocab"] >= 51865

    @property
    def precision(self) -> str:
        return self.encoder.precision

    def set_precision(self, precision: str) -> "Whisper":
        """The audio encoder's precision (``AudioEncoder.set_precision``: ``"fp32"`` | ``"bf16x3"``); the decoder is exact fp32 always"""
        self.encoder.set_precision(precision)
        return self

    def embed_audio(self, mel: torch.Tensor) -> torch.Tensor:
        return self.encoder(mel)

    def logits(self, tokens: torch.Tensor, audio_features: torch.Tensor) -> torch.Tensor:
        return self.decoder(tokens, audio_features)

    def forward(self, mel: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
        return self.decoder(tokens, self.encoder(mel))

    def decode(self, mel, options: DecodingOptions = DecodingOptions(), *, graph: Optional[bool] = None):
        return decode(self, mel, options, graph=graph)

    def graph_stats(self) -> Dict[str, int]:
        """Counts since the model was made: ``captures`` (hipGraphs captured by the replayed decoding loop), ``replays`` (chunks
        replayed) and ``eager_steps`` (loop iterations issued launch by launch, those of loops without ``graph`` included)"""
        return dict(self.decoder.graph_stats)

    def detect_language(self, mel, tokenizer: Optional[Tokenizer] = None):
        return detect_language(self, mel, tokenizer)

    def transcribe(self, audio, **kw):
        return transcribe(self, audio, **kw)

    def transcribe_many(self, audios, **kw):
        return transcribe_many(self, audios, **kw)


def load_model(path: str, device: Optional[Union[str, torch.device]] = None, tokenizer: Optional[Union[str, Tokenizer]] = None, *,
               precision: Optional[str] = None) -> Whisper:
    """A local OpenAI ``.pt`` checkpoint or a Hugging Face model directory -> ``Whisper``.  There are no model names and no downloads: a
    bare name (``'small.en'``) raises FileNotFoundError saying so.  ``tokenizer``: a ``Tokenizer`` or a directory with ``vocab.json`` and
    ``merges.txt`` (default: the model directory itself when it has them; a ``.pt`` carries no vocabulary).  ``precision``: the audio
    encoder's (``Whisper.set_precision``; default: the environment's ``HIREST_WHISPER_PRECISION``, else ``"fp32"``)."""
    dims, sd, is_dir = _read_checkpoint(path, ": model names are not resolved and nothing is downloaded (no network access) — download "
                                              "the model beforehand and pass its path")
    model = Whisper(dims, sd).set_precision(_load_precision(precision))
    if is_dir and tokenizer is None and os.path.isfile(os.path.join(path, "vocab.json")):
        tokenizer = path
    if isinstance(tokenizer, (str, os.PathLike)):
        multilingual = model.is_multilingual
        tokenizer = Tokenizer.from_dir(os.fspath(tokenizer), language="en" if multilingual else None, task="transcribe" if multilingual else None)
    model.tokenizer = tokenizer
    return model.to(device) if device is not None else model


class _FileWalk:
    """``transcribe()``'s walk over one file, cut at its decode calls so that one caller can drive one file with ``decode`` and another
    the current windows of several files with ``decode_many``: ``next_request()`` is the next (window, options) to decode, or None when
    the file is done; ``accept(result)`` takes that request's result — it moves on to the next fallback temperature of the same window
    or settles the window (no-speech skip, segments, ``seek``, prompt reset); ``result()`` is ``transcribe()``'s dict."""

    def __init__(self, model, audio, *, temperature: Union[float, Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                 compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                 no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True, initial_prompt: Optional[str] = None,
                 verbose=None, word_timestamps: bool = False, prepend_punctuations: str = PREPEND_PUNCTUATIONS,
                 append_punctuations: str = APPEND_PUNCTUATIONS, **decode_options):
        self.word_timestamps, self.punctuations = bool(word_timestamps), (prepend_punctuations, append_punctuations)
        self.tokenizer = tokenizer = decode_options.pop("tokenizer", None) or getattr(model, "tokenizer", None)
        if tokenizer is None:
            raise ValueError("no tokenizer: load_model(path, tokenizer=...) or transcribe(..., tokenizer=...)")
        # A multilingual tokenizer (``Tokenizer.multilingual``): the code of ``language=`` — a code, name or alias — or None until
        # ``_detect_file_languages`` has looked at the file's first window.  English-only: "en" whatever was asked.
        self.model, self.multilingual = model, tokenizer.multilingual
        language = decode_options.get("language")
        self.language = (language_code(language) if language is not None else None) if self.multilingual else "en"
        dims = model.dims
        if torch.is_tensor(audio) and audio.ndim == 2:
            self.mel = audio
        else:
            self.mel = log_mel_spectrogram(audio, dims["n_mels"], padding=N_SAMPLES, device=model.device)
        self.content_frames = self.mel.shape[-1] - N_FRAMES
        self.input_stride = N_FRAMES // dims["n_audio_ctx"]           # mel frames per encoder position: 2
        self.time_precision = self.input_stride * HOP_LENGTH / SAMPLE_RATE      # 0.02 s per timestamp token
        self.temperatures = (temperature,) if isinstance(temperature, (int, float)) else tuple(temperature)
        self.compression_ratio_threshold, self.logprob_threshold = compression_ratio_threshold, logprob_threshold
        self.no_speech_threshold, self.condition_on_previous_text = no_speech_threshold, condition_on_previous_text
        self.decode_options = decode_options
        self.seek, self.all_tokens, self.all_segments, self.reset_since = 0, [], [], 0
        self.attempt = 0                                              # index of the fallback temperature the current window is at
        if initial_prompt is not None:
            self.all_tokens.extend(tokenizer.encode(" " + initial_prompt.strip()))

    @property
    def finished(self) -> bool:
        return self.seek >= self.content_frames

    def first_window(self) -> torch.Tensor:
        return pad_or_trim(self.mel[:, :N_FRAMES], N_FRAMES)

    def next_request(self):
        if self.finished:
            return None
        t = self.temperatures[self.attempt]
        kw = dict(self.decode_options)
        kw["prompt"] = self.all_tokens[self.reset_since:]
        if self.multilingual:
            if self.language is None:                                 # (nobody detected it together with other files')
                _detect_file_languages(self.model, [self])
            kw["language"] = self.language                            # every window of the file decodes in the file's language
        for k in (("beam_size", "patience") if t > 0 else ("best_of",)):      # the sampling branch has no beams, the greedy one no candidates
            kw.pop(k, None)
        return pad_or_trim(self.mel[:, self.seek:self.seek + N_FRAMES], N_FRAMES), DecodingOptions(**kw, temperature=float(t))

    def _add_segment(self, start: float, end: float, tokens: List[int], result: DecodingResult):
        text = self.tokenizer.decode([t for t in tokens if t < self.tokenizer.eot])
        if not text.strip():
            return
        self.all_segments.append({"id": len(self.all_segments), "seek": self.seek, "start": start, "end": end, "text": text,
                                  "tokens": list(tokens), "temperature": result.temperature, "avg_logprob": result.avg_logprob,
                                  "compression_ratio": result.compression_ratio, "no_speech_prob": result.no_speech_prob})
        self.all_tokens.extend(tokens)

    def accept(self, result: DecodingResult) -> None:
        again = self.compression_ratio_threshold is not None and result.compression_ratio > self.compression_ratio_threshold
        again = again or (self.logprob_threshold is not None and result.avg_logprob < self.logprob_threshold)
        if again and self.attempt + 1 < len(self.temperatures):
            self.attempt += 1                                         # the same window again, at the next temperature
            return
        self.attempt = 0
        tb, seek, input_stride, time_precision = self.tokenizer.timestamp_begin, self.seek, self.input_stride, self.time_precision
        add_segment, logprob_threshold = self._add_segment, self.logprob_threshold
        window_start = seek
        time_offset = seek * HOP_LENGTH / SAMPLE_RATE
        segment_size = min(N_FRAMES, self.content_frames - seek)
        tokens = list(result.tokens)
        if self.no_speech_threshold is not None and result.no_speech_prob > self.no_speech_threshold and \
                not (logprob_threshold is not None and result.avg_logprob > logprob_threshold):
            self.seek = seek + segment_size                           # silence: skip the window
            return
        n_before = len(self.all_segments)
        is_ts = [t >= tb for t in tokens]
        single_ending = is_ts[-2:] == [False, True]
        cuts = [i + 1 for i in range(len(tokens) - 1) if is_ts[i] and is_ts[i + 1]]
        if cuts:
            if single_ending:
                cuts.append(len(tokens))
            last = 0
            for cut in cuts:
                piece = tokens[last:cut]
                add_segment(time_offset + (piece[0] - tb) * time_precision, time_offset + (piece[-1] - tb) * time_precision, piece, result)
                last = cut
            if single_ending:
                seek += segment_size                                  # a single timestamp at the end: no speech after it
            else:
                seek += (tokens[last - 1] - tb) * input_stride        # the rest of the window is decoded again from the last pair's end
        else:
            duration = segment_size * HOP_LENGTH / SAMPLE_RATE
            stamps = [t for t in tokens if t >= tb]
            if stamps and stamps[-1] != tb:
                duration = (stamps[-1] - tb) * time_precision
            add_segment(time_offset, time_offset + duration, tokens, result)
            seek += segment_size
        if seek <= window_start:                                      # (a last pair that closes at <|0.00|>, possible only without the
            seek = window_start + segment_size                        #  monotonic rule, would decode the same window for ever)
        if self.word_timestamps and len(self.all_segments) > n_before:
            # One alignment per settled window, on the window's own states when decode() handed them back.  ``seek`` stays where the
            # timestamp tokens put it (Whisper moves it to the last word's end; here every field but "words" is what it is without).
            states = result.audio_features
            if states is None:
                states = pad_or_trim(self.mel[:, window_start:window_start + N_FRAMES], N_FRAMES)
            tok = self.tokenizer
            if self.multilingual:
                task = self.decode_options.get("task", "transcribe")
                tok = tok.with_language(self.language, task if task != "transcribe" else tok.task or "transcribe")
            # (a file's last sliver of one frame still has the one key its words are put at)
            add_word_timestamps(self.all_segments[n_before:], self.model, tok, states, max(segment_size, 2), prepend_punctuations=self.punctuations[0],
                                append_punctuations=self.punctuations[1])
        self.seek = seek                                              # (after the segments: they carry the window's own seek)
        if not self.condition_on_previous_text or result.temperature > 0.5:
            self.reset_since = len(self.all_tokens)

    def result(self) -> Dict[str, object]:
        if self.multilingual and self.language is None:               # a file without a window to decode still names its language
            _detect_file_languages(self.model, [self])
        text_tokens = [t for s in self.all_segments for t in s["tokens"] if t < self.tokenizer.eot]
        return {"text": self.tokenizer.decode(text_tokens), "segments": self.all_segments, "language": self.language}


def _detect_file_languages(model, walks) -> None:
    """Whisper's rule, once per file and not per window: a file of a multilingual model whose ``language`` is None takes the language
    detected on its first 30 seconds.  All of ``walks`` that still wait for theirs go through ONE ``detect_language`` call."""
    waiting = [w for w in walks if w.multilingual and w.language is None]
    if not waiting:
        return
    tokenizer = waiting[0].tokenizer
    tokens, _ = detect_language(model, torch.stack([w.first_window() for w in waiting]), tokenizer)
    for w, token in zip(waiting, tokens.tolist()):
        w.language = tokenizer.all_language_codes[tokenizer.all_language_tokens.index(token)]


def transcribe(model, audio, *, graph: Optional[bool] = None, **kw):
    """``whisper.transcribe``: a ``.wav`` path, a waveform or a ready spectrogram ``[n_mels, frames]`` (with its 30 s of padding) ->
    ``{"text", "segments", "language"}``.  One spectrogram per file; 3000-frame windows from ``seek``; per window the temperature
    fallback (the next temperature when the compression ratio or the average log-probability crosses its threshold), the no-speech
    skip, segments cut at consecutive timestamp pairs, ``seek`` advanced to the last timestamp or by the whole window; the prompt of
    the next window is the text so far, reset after a window decoded above temperature 0.5.  Keywords: ``temperature`` (one or a tuple,
    default 0.0 .. 1.0 in steps of 0.2), ``compression_ratio_threshold`` (2.4), ``logprob_threshold`` (-1.0), ``no_speech_threshold``
    (0.6), ``condition_on_previous_text`` (True), ``initial_prompt``, ``verbose``, ``tokenizer``; the rest are ``DecodingOptions``.
    ``word_timestamps=True`` (with ``prepend_punctuations`` / ``append_punctuations``, Whisper's defaults): every settled window that
    yielded segments is aligned once (``add_word_timestamps``: one teacher-forced pass) and each of its segments gains
    ``"words": [{"word", "start", "end", "probability"}]``; ``seek``, tokens, text and every other field are what they are without the
    option — Whisper moves ``seek`` to the last word's end, which is deliberately not done here.
    With a multilingual model ``language`` is a code, name or alias, or None: the language detected on the file's first 30 seconds
    (``detect_language``, once per file) — every window decodes in it and the result's ``"language"`` is its code; ``task`` is
    "transcribe" or "translate".  An English-only model ignores both: ``"language"`` is "en".  ``graph`` as ``decode``'s: every window's
    loop is replayed from a captured hipGraph."""
    graph = {"graph": True} if resolve_graph(graph) else {}
    walk = _FileWalk(model, audio, **kw)
    while True:
        request = walk.next_request()
        if request is None:
            return walk.result()
        walk.accept(decode(model, *request, **graph))


def transcribe_many(model, audios, *, files_in_flight: int = FILES_IN_FLIGHT, graph: Optional[bool] = None, **kw):
    """``transcribe()`` of every item of ``audios`` (keywords as ``transcribe``'s, the same for all), with the current windows of up
    to ``files_in_flight`` files decoded together by ``decode_many``: a file's windows stay in order, files are independent.  After a
    round every file takes its result (a fallback is simply its request of the next round); a file that ends hands its slot to the
    next one.  The files that take a slot in the same round and name no language (a multilingual model, ``language=None``) have their
    first windows detected in one ``detect_language`` call (a file without content never takes a slot: its language is detected by a
    call of its own when its result is taken).  Returns the files' dicts in input order, each equal to ``transcribe()``'s."""
    if files_in_flight < 1:
        raise ValueError(f"files_in_flight = {files_in_flight}: at least one file")
    graph = {"graph": True} if resolve_graph(graph) else {}
    audios = list(audios)
    out: List[Optional[Dict[str, object]]] = [None] * len(audios)
    waiting = iter(range(len(audios)))

    def seat(walk_of_slot):
        """the slot's (file index, its walk) while it has windows left; a finished file hands the slot to the next waiting one"""
        while True:
            if walk_of_slot is None:
                i = next(waiting, None)
                if i is None:
                    return None
                walk_of_slot = (i, _FileWalk(model, audios[i], **kw))
            i, walk = walk_of_slot
            if not walk.finished:
                return walk_of_slot
            out[i] = walk.result()
            walk_of_slot = None

    def seat_all(slots):
        slots = [seat(s) for s in slots]
        _detect_file_languages(model, [s[1] for s in slots if s is not None])          # the newly seated files' languages, together
        return slots
    slots = seat_all([None] * files_in_flight)
    while any(s is not None for s in slots):
        live = [s for s in slots if s is not None]
        requests = [walk.next_request() for _, walk in live]
        results = decode_many(model, [r[0] for r in requests], [r[1] for r in requests], **graph)
        for (_, walk), result in zip(live, results):
            walk.accept(result)
        slots = seat_all(slots)
    return out


def format_timestamp(seconds: float, always_include_hours: bool = False, decimal_marker: str = ".") -> str:
    if seconds < 0:
        raise ValueError("non-negative timestamp expected")
    ms = int(round(seconds * 1000.0))
    h, ms = divmod(ms, 3_600_000)
    m, ms = divmod(ms, 60_000)
    s, ms = divmod(ms, 1000)
    hours = f"{h:02d}:" if always_include_hours or h > 0 else ""
    return f"{hours}{m:02d}:{s:02d}{decimal_marker}{ms:03d}"


def write_srt(segments, file) -> None:
    """Segments of ``transcribe()`` as SubRip: index, ``HH:MM:SS,mmm --> HH:MM:SS,mmm``, text, blank line (what ``dataset.read_srt_spans``
    and the ``srt`` package parse)."""
    for i, seg in enumerate(segments, start=1):
        print(f"{i}\n{format_timestamp(seg['start'], True, ',')} --> {format_timestamp(seg['end'], True, ',')}\n"
              f"{seg['text'].strip().replace('-->', '->')}\n", file=file, flush=True)


utils = types.SimpleNamespace(write_srt=write_srt, format_timestamp=format_timestamp)


# ---------------------------------------------------------------------------------------------------------------------------------
# word-level timestamps (whisper/timing.py's names)
# ---------------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class WordTiming:
    word: str
    tokens: List[int]
    start: float
    end: float
    probability: float


def median_filter(x: torch.Tensor, width: int) -> torch.Tensor:
    """``whisper.timing.median_filter``: a median filter of odd ``width`` (at most 31) along the last axis of a device tensor, reflect
    padding of ``width // 2`` on both sides; a last axis of at most ``width // 2`` elements comes back unfiltered (Whisper's early
    return).  fp32; the median is selected, so the values are exact."""
    if width < 1 or width % 2 != 1:
        raise ValueError(f"width {width}: an odd filter width expected")
    dev = _gpu_device(x.device, "median_filter")
    w = x.to(torch.float32).contiguous()
    n = int(w.shape[-1])
    rows = w.numel() // max(n, 1)
    if w.numel() == 0:
        return w.clone()
    out = torch.empty_like(w)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hirest_median_filter_mean_f32(w.data_ptr(), 1, rows, n, int(width), 0, rows, out.data_ptr(), ops.stream_ptr()),
                   "hirest_median_filter_mean_f32")
    return out


def dtw_many(xs, *, negate: bool = False, return_cost: bool = False):
    """``dtw`` of several matrices in one launch (one workgroup each): a list of ``(text_indices, time_indices)``, with ``return_cost``
    of ``(text_indices, time_indices, cost [N, M] on the device)``.  ``negate``: of ``-x`` without forming it."""
    lib = _lib.load()
    if not xs:
        return []
    dev = _gpu_device(xs[0].device, "dtw")
    xs = [x if x.dtype == torch.float32 and x.stride(-1) == 1 else x.to(torch.float32).contiguous() for x in xs]
    probs = (_lib.DtwProblem * len(xs))()
    keep = []
    for p, x in zip(probs, xs):
        if x.ndim != 2 or not (1 <= x.shape[0] <= _lib.DTW_MAX_N and 1 <= x.shape[1] <= _lib.DTW_MAX_M):
            raise ValueError(f"dtw of a matrix of shape {tuple(x.shape)}: [N <= {_lib.DTW_MAX_N}, M <= {_lib.DTW_MAX_M}] expected")
        N, M = int(x.shape[0]), int(x.shape[1])
        path = torch.empty((N + M + 1, 2), dtype=torch.int32, device=dev)          # the last row's first word: the path's length
        cost = torch.empty((N, M), dtype=torch.float32, device=dev) if return_cost else None
        p.x, p.ldx, p.N, p.M, p.negate = x.data_ptr(), x.stride(0) if N > 1 else M, N, M, int(negate)
        p.path, p.path_len = path.data_ptr(), path[N + M].data_ptr()
        p.cost, p.ldc = (cost.data_ptr(), M) if return_cost else (None, 0)
        keep.append((path, cost))
    with torch.cuda.device(dev):
        ws = torch.empty((int(lib.hirest_dtw_workspace_bytes(probs, len(xs))),), dtype=torch.uint8, device=dev)
        _lib.check(lib.hirest_dtw_f32(probs, len(xs), ws.data_ptr(), ws.numel(), ops.stream_ptr()), "hirest_dtw_f32")
        out = []
        for path, cost in keep:
            host = path.cpu().numpy()                                              # one read-back per problem: the path and its length
            steps = host[:int(host[-1, 0])]
            out.append((steps[:, 0].copy(), steps[:, 1].copy()) + ((cost,) if return_cost else ()))
    return out


def dtw(x: torch.Tensor):
    """``whisper.timing.dtw``: the minimum-cost monotone path through ``x [N, M]`` (a device tensor, N <= 256, M <= 4096) as
    ``(text_indices, time_indices)``, numpy arrays.  Recurrence and backtrace run on the device (``hirest_dtw_f32``); ties go the way
    Whisper's go (diagonal only when strictly smallest, then up only when strictly smallest, else left)."""
    return dtw_many([x])[0]


def alignment_matrix(queries, cross_kv, pairs, n_keys: int, *, heads: int, qk_scale: float = 1.0, medfilt_width: int = 7, row0: int = 0,
                     n_rows: Optional[int] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hirest_whisper_alignment_matrix`` for one window: ``queries`` per layer the cross-attention query rows ``[T, D]``, ``cross_kv``
    per layer the window's ``key | value`` rows ``[Tk, 2 D]``, ``pairs`` the selected (layer, head) -> fp32 ``[n_rows, n_keys]``: the
    selected heads' softmax over the first ``n_keys`` keys, normalised per key over the T tokens, median-filtered along the keys,
    averaged over the heads."""
    lib = _lib.load()
    layers, T, Tk = len(queries), int(queries[0].shape[0]), int(cross_kv[0].shape[0])
    dev = _gpu_device(queries[0].device, "alignment_matrix")
    n_rows = T - row0 if n_rows is None else n_rows
    pairs = [(int(l), int(h)) for l, h in pairs]
    for t in list(queries) + list(cross_kv):
        if t.dtype != torch.float32 or t.stride(-1) != 1:
            raise ValueError("fp32 rows with unit stride expected")
    P = C.c_void_p * layers
    q_ptrs, kv_ptrs = P(*(t.data_ptr() for t in queries)), P(*(t.data_ptr() for t in cross_kv))
    sel = (C.c_int32 * (2 * len(pairs)))(*(v for pair in pairs for v in pair))
    need = int(lib.hirest_whisper_alignment_workspace_bytes(len(pairs), T, n_keys))
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
        out = torch.empty((max(n_rows, 0), max(n_keys, 0)), dtype=torch.float32, device=dev)
        _lib.check(lib.hirest_whisper_alignment_matrix(q_ptrs, queries[0].stride(0), kv_ptrs, layers, heads, Tk, sel, len(pairs), T, n_keys,
                                                       float(qk_scale), int(medfilt_width), row0, n_rows, out.data_ptr(), workspace.data_ptr(),
                                                       workspace.numel(), ops.stream_ptr()), "hirest_whisper_alignment_matrix")
    return out


def _split_words(tokenizer: Tokenizer, text_tokens: List[int], segment_lengths=None):
    """Whisper's ``split_to_word_tokens(text_tokens + [eot])`` — or, given the segments' token counts, the same per segment, so that
    no word spans two segments"""
    if not segment_lengths:
        return tokenizer.split_to_word_tokens(list(text_tokens) + [tokenizer.eot])
    if sum(segment_lengths) != len(text_tokens):
        raise ValueError(f"segment lengths {list(segment_lengths)} for {len(text_tokens)} text tokens")
    words, word_tokens, at = [], [], 0
    for k, n in enumerate(segment_lengths):
        piece = list(text_tokens[at:at + n]) + ([tokenizer.eot] if k == len(segment_lengths) - 1 else [])
        at += n
        if piece:
            w, t = tokenizer.split_to_word_tokens(piece)
            words += w
            word_tokens += t
    return words, word_tokens


def words_from_path(words, word_tokens, text_indices, time_indices, token_probs) -> List[WordTiming]:
    """steps 6 to 8 of ``find_alignment``: the times at which the path enters a new token, the words' boundaries among them"""
    boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    jump_times = time_indices[jumps] / TOKENS_PER_SECOND
    starts, ends = jump_times[boundaries[:-1]], jump_times[boundaries[1:]]
    probs = [float(np.mean(token_probs[i:j])) for i, j in zip(boundaries[:-1], boundaries[1:])]
    return [WordTiming(w, list(t), float(s), float(e), p) for w, t, s, e, p in zip(words, word_tokens, starts, ends, probs)]


@torch.no_grad()
def find_alignment(model: "Whisper", tokenizer: Tokenizer, text_tokens: List[int], mel_or_states: torch.Tensor, num_frames: int, *,
                   medfilt_width: int = 7, qk_scale: float = 1.0, segment_lengths=None, details: Optional[dict] = None) -> List[WordTiming]:
    """``whisper.timing.find_alignment``: the words of ``text_tokens`` (text ids only) with the times at which one window's audio
    (``[n_mels, 3000]``, or its encoder states ``[Tk, D]``) says them.  One teacher-forced pass of ``sot_sequence, <|notimestamps|>,
    text, eot`` keeps every layer's cross-attention queries; ``hirest_whisper_alignment_matrix`` turns those of ``model.
    alignment_heads`` into the ``[len(text) + 1, num_frames // 2]`` matrix; ``dtw`` of its negative gives the path; a word starts
    and ends where the path enters its first token and the next word's.  ``probability`` is the mean over the word's tokens of the
    softmax, over the text ids (columns below eot, as Whisper takes them), of the logits that predict them.  At most one word
    (the text's words and eot's): an empty list.  ``segment_lengths``: see ``add_word_timestamps``.  ``details``: a dict that
    receives the matrix, the path and the token probabilities (tests)."""
    text_tokens = [int(t) for t in text_tokens]
    if not text_tokens:
        return []
    words, word_tokens = _split_words(tokenizer, text_tokens, segment_lengths)
    if len(word_tokens) <= 1:
        return []
    dec, dev = model.decoder, model.device
    sot = list(tokenizer.sot_sequence)
    tokens = sot + [tokenizer.no_timestamps] + text_tokens + [tokenizer.eot]
    T, n = len(tokens), len(text_tokens)
    if T > dec.ctx:
        raise ValueError(f"{n} text tokens make a sequence of {T}: the decoder has {dec.ctx} positions")
    if n + 1 > _lib.DTW_MAX_N:
        raise ValueError(f"{n} text tokens: the alignment takes up to {_lib.DTW_MAX_N - 1}")
    states = mel_or_states if mel_or_states.ndim == 3 else mel_or_states[None]
    with torch.cuda.device(dev):
        xa = _audio_states(model, states)[:1]
        Tk = int(xa.shape[1])
        n_keys = int(num_frames) // 2
        if not 1 <= n_keys <= min(Tk, _lib.DTW_MAX_M):
            raise ValueError(f"num_frames {num_frames}: between 2 and {2 * min(Tk, _lib.DTW_MAX_M)} expected")
        cross_kv = dec.cross_kv(xa)
        queries: List[torch.Tensor] = []
        x = dec._sequences(torch.tensor([tokens], dtype=torch.int32), cross_kv, Tk, keep_cross_q=lambda i, q: queries.append(q))
        logits = dec._head(x)[len(sot):len(sot) + n, :tokenizer.eot]
        ids = torch.tensor(text_tokens, dtype=torch.int64, device=dev)
        token_probs = torch.softmax(logits, dim=-1).gather(1, ids[:, None])[:, 0]
        pairs = model.alignment_heads.nonzero().tolist()
        matrix = alignment_matrix(queries, [kv[0] for kv in cross_kv], pairs, n_keys, heads=dec.heads, qk_scale=qk_scale,
                                  medfilt_width=medfilt_width, row0=len(sot), n_rows=n + 1)
        (text_indices, time_indices), = dtw_many([matrix], negate=True)
        token_probs = token_probs.cpu().numpy()
    if details is not None:
        details.update(matrix=matrix, text_indices=text_indices, time_indices=time_indices, token_probs=token_probs, words=words,
                       word_tokens=word_tokens)
    return words_from_path(words, word_tokens, text_indices, time_indices, token_probs)


def merge_punctuations(alignment: List[WordTiming], prepended: str = PREPEND_PUNCTUATIONS, appended: str = APPEND_PUNCTUATIONS) -> None:
    """``whisper.timing.merge_punctuations``, in place: a word that is a space and a ``prepended`` character joins the word after it,
    a word that is an ``appended`` character joins the word before it (unless that ends with a space); the joined word keeps its own
    times, the absorbed one is left with an empty word and no tokens."""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:
        previous, following = alignment[i], alignment[j]
        if previous.word.startswith(" ") and previous.word.strip() in prepended:
            following.word = previous.word + following.word
            following.tokens = previous.tokens + following.tokens
            previous.word, previous.tokens = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        previous, following = alignment[i], alignment[j]
        if not previous.word.endswith(" ") and following.word in appended:
            previous.word = previous.word + following.word
            previous.tokens = previous.tokens + following.tokens
            following.word, following.tokens = "", []
        else:
            i = j
        j += 1


def add_word_timestamps(segments, model: "Whisper", tokenizer: Tokenizer, mel: torch.Tensor, num_frames: int, *,
                        prepend_punctuations: str = PREPEND_PUNCTUATIONS, append_punctuations: str = APPEND_PUNCTUATIONS, **kwargs) -> None:
    """``whisper.timing.add_word_timestamps`` for the segments of ONE window (``mel``: the window, or its encoder states): one
    ``find_alignment`` over the window's text tokens, the punctuations merged, the words handed to the segments by token count, the
    window's time offset (``segments[0]["seek"]``) added and times rounded to 1/100 s; each segment gains ``"words"``.

    Where this differs from Whisper, on purpose: words are split per segment and punctuation merges inside a segment, so a word never
    spans two segments and a segment's words concatenate to its text; the segment's bounds are kept and the words' times are clipped
    into them (Whisper moves the segment's bounds to its words); Whisper's median-duration clamps on long words and its
    pause heuristics are NOT built."""
    segments = list(segments)
    if not segments:
        return
    per_segment = [[t for t in s["tokens"] if t < tokenizer.eot] for s in segments]
    text_tokens = [t for tokens in per_segment for t in tokens]
    alignment = find_alignment(model, tokenizer, text_tokens, mel, num_frames, segment_lengths=[len(t) for t in per_segment], **kwargs)
    offset = segments[0]["seek"] * HOP_LENGTH / SAMPLE_RATE
    at = 0
    for segment, tokens in zip(segments, per_segment):
        first, saved = at, 0
        while at < len(alignment) and saved < len(tokens):
            saved += len(alignment[at].tokens)
            at += 1
        mine = alignment[first:at]
        merge_punctuations(mine, prepend_punctuations, append_punctuations)
        lo, hi = segment["start"], segment["end"]
        segment["words"] = [{"word": w.word, "start": min(max(round(offset + w.start, 2), lo), hi), "end": min(max(round(offset + w.end, 2), lo), hi),
                             "probability": w.probability} for w in mine if w.word]


timing = types.SimpleNamespace(median_filter=median_filter, dtw=dtw, dtw_many=dtw_many, alignment_matrix=alignment_matrix,
                               find_alignment=find_alignment, merge_punctuations=merge_punctuations, add_word_timestamps=add_word_timestamps,
                               WordTiming=WordTiming)
