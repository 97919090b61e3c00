#!/usr/bin/env python
"""The fixture of Whisper's language detection: tests/golden/whisper_lang.npz.

As tests/golden/make_whisper_dec_golden.py: ``transformers``' WhisperDecoder in float64 on the CPU, on ``hirest_amd.synth``'s seeded
weights of decoder case q with the four language tokens of tests/_whisper_lang.py (which also says why the ``<|en|>`` row is scaled).
It holds, for the windows of ``_whisper_lang.audio_states("q")``, the fp64 logits of the ``<|startoftranscript|>`` position — what
``detect_language`` looks at —, the fp64 softmax over the language columns, the winners, and the two yardsticks of the same forward run
in fp32 on the CPU: the largest error of a logit and the largest error of a probability; and the same position's ``no_speech_prob``
(the softmax over the whole vocabulary at ``<|nospeech|>``) with its fp32 yardstick, which ``decode()`` must still read there.

The fixture is refused when a window's top-2 margin among the language columns is below 100 x the fp32 forward's error (the winner
would then be excused), and when fewer than two languages win over the windows (a constant answer would pass).

    python tests/golden/make_whisper_lang_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _whisper_lang as L  # noqa: E402
from hirest_amd import synth  # noqa: E402
from make_whisper_dec_golden import hf_decoder, logits_of  # noqa: E402

CASE = "q"


def main():
    cfg, eot, _, _ = synth.WHISPER_DEC_CASES[CASE]
    sd = L.decoder_state_dict(CASE)
    dec64, dec32 = hf_decoder(cfg, sd, torch.float64), hf_decoder(cfg, sd, torch.float32)
    emb = sd["decoder.embed_tokens.weight"].double()
    tok = L.tokenizer(eot)
    ids = list(tok.all_language_tokens)
    xa = L.audio_states(CASE)
    W = int(xa.shape[0])
    sot = torch.full((W, 1), tok.sot, dtype=torch.int64)
    _, l64 = logits_of(dec64, emb, sot, xa.double())
    _, l32 = logits_of(dec32, emb.float(), sot, xa)
    l64, l32 = l64[:, 0].numpy(), l32[:, 0].numpy()
    err = float(np.abs(l32.astype(np.float64) - l64).max())
    p64 = L.masked_softmax(l64, ids, np.float64)
    p32 = L.masked_softmax(l32, ids, np.float32)
    perr = float(np.abs(p32.astype(np.float64) - p64).max())
    # no_speech_prob, which decode() reads from the same position: the softmax over the whole vocabulary at <|nospeech|>
    ns64 = L.masked_softmax(l64, range(cfg["vocab_size"]), np.float64)[:, tok.no_speech]
    ns32 = L.masked_softmax(l32, range(cfg["vocab_size"]), np.float32)[:, tok.no_speech]
    nserr = float(np.abs(ns32.astype(np.float64) - ns64).max())
    cols = np.sort(l64[:, ids], axis=-1)
    margins = cols[:, -1] - cols[:, -2]
    winners = np.array([ids[j] for j in l64[:, ids].argmax(-1)], dtype=np.int32)
    codes = [tok.all_language_codes[ids.index(int(t))] for t in winners]
    print(f"{CASE}: {W} windows, winners {codes}, margins {np.round(margins, 4).tolist()}, fp32 CPU error: logits {err:.3e}, probabilities {perr:.3e}")
    if float(margins.min()) < 100 * err:
        raise SystemExit(f"a window's margin {float(margins.min()):.3e} is below 100 x the fp32 error {err:.3e}: choose other seeds")
    if len(set(codes)) < 2:
        raise SystemExit(f"every window detects {codes[0]}: a constant answer would pass; choose other seeds or bias the language rows")
    if W < 4:
        raise SystemExit(f"{W} windows: at least 4")
    path = os.path.join(HERE, "whisper_lang.npz")
    np.savez_compressed(path, logits64=l64, probs64=p64, winners=winners, margins=margins, err32=np.float64(err), probs_err32=np.float64(perr),
                        no_speech64=ns64, no_speech_err32=np.float64(nserr))
    print(f"  wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
