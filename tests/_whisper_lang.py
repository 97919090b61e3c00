"""What the language tests share (tests/test_gpu_whisper_language.py, tests/test_whisper_language_host.py) with the script that writes
their fixture (tests/golden/make_whisper_lang_golden.py): the synthetic multilingual tokenizer — synth's vocabulary of a decoder case plus
four language tokens in the free slots eot + 2 .. eot + 5 — the decoder weights, and the fixture's windows.

With the plain seeded weights every window of case q prefers ``<|en|>`` by 0.05 to 0.3 (its embedding row happens to lie along the
states of the ``<|startoftranscript|>`` position), and a test of detection against a constant answer shows nothing.  So the ``<|en|>``
row of the embedding — also the LM head's — is scaled by 0.85 here: its logit drops among those of ``<|zh|>`` and ``<|de|>`` and the
windows' audio decides.  The fixture script refuses a set of windows with fewer than two winners."""
import numpy as np
import torch

from hirest_amd import synth, whisper

LANGS = ("en", "zh", "de", "es")
EN_ROW_SCALE = 0.85
WINDOW_SEEDS = 3               # the fixture's windows: the case's own audio-state seed and the next ones, the case's window count from each


def special_tokens(eot: int, langs=LANGS):
    sp = synth.whisper_special_tokens(eot)
    sp.update({f"<|{code}|>": eot + 2 + i for i, code in enumerate(langs)})
    return sp


def tokenizer(eot: int, language="en", task="transcribe"):
    return whisper.Tokenizer(*synth.whisper_vocab(eot), special_tokens(eot), language=language, task=task)


def decoder_state_dict(case: str):
    cfg, eot, seed, _ = synth.WHISPER_DEC_CASES[case]
    sd = synth.whisper_decoder_state_dict(cfg, seed, eot, synth.WHISPER_DEC_EOT_BIAS[case])
    sd["decoder.embed_tokens.weight"][eot + 2] *= EN_ROW_SCALE
    return sd


def audio_states(case: str) -> torch.Tensor:
    """[WINDOW_SEEDS * windows, Tk, D]: the first ``windows`` are the case's own (tests/golden/whisper_dec_<case>.npz)"""
    cfg, _, seed, windows = synth.WHISPER_DEC_CASES[case]
    return torch.cat([synth.whisper_audio_states(cfg, windows, seed + 100 + k) for k in range(WINDOW_SEEDS)])


def model_for(case: str, dev, enc_cfg=None, language="en", task="transcribe"):
    """the case's decoder behind a small synthetic encoder, with the multilingual tokenizer"""
    cfg, eot, _, _ = synth.WHISPER_DEC_CASES[case]
    cfg = {**cfg, **(enc_cfg or {})}
    enc = synth.whisper_encoder_state_dict(cfg, 73)
    sd = {**{"encoder." + k: v for k, v in enc.items()}, **decoder_state_dict(case)}
    return whisper.Whisper(cfg, sd, tokenizer(eot, language, task)).to(dev)


def masked_softmax(logits: np.ndarray, ids, dtype=np.float64) -> np.ndarray:
    """the kernel's formula restated: exp(x - max) / sum over the columns ``ids`` of rows of logits, summed in ascending order in ``dtype``"""
    x = np.asarray(logits)[..., list(ids)].astype(dtype)
    e = np.exp(x - x.max(-1, keepdims=True)).astype(dtype)
    s = np.zeros(e.shape[:-1], dtype=dtype)
    for j in range(e.shape[-1]):
        s = (s + e[..., j]).astype(dtype)
    return (e / s[..., None]).astype(dtype)
