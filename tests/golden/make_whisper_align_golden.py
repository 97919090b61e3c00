#!/usr/bin/env python
"""Fixtures of the word alignment's token probabilities: tests/golden/whisper_align_{p,q,s}.npz.

``find_alignment`` runs ``<|startoftranscript|>, <|notimestamps|>, text, <|endoftext|>`` through the decoder and takes, for every text
token, the softmax over the text ids (columns below eot) of the logits that predict it.  The yardstick is ``transformers``'
WhisperDecoder in float64 on ``hirest_amd.synth``'s seeded weights, as for tests/golden/whisper_dec_*.npz; the error of the same
softmax rows in fp32 on the CPU (the largest over their entries) is the tests' bar.  Per case two texts: ``greedy`` (the text ids of the case's greedy fixture, what decode() returns for
window 0) and ``extra`` (the text ids of the case's 9-token prompt fixture, so that case p, whose greedy text is empty, aligns something).

    python tests/golden/make_whisper_align_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hirest_amd import synth  # noqa: E402
from make_whisper_dec_golden import hf_decoder, logits_of  # noqa: E402


def main():
    for case in ("p", "q", "s"):
        cfg, eot, seed, windows = synth.WHISPER_DEC_CASES[case]
        sd = synth.whisper_decoder_state_dict(cfg, seed, eot, synth.WHISPER_DEC_EOT_BIAS[case])
        dec64, dec32 = hf_decoder(cfg, sd, torch.float64), hf_decoder(cfg, sd, torch.float32)
        emb = sd["decoder.embed_tokens.weight"].double()
        xa = synth.whisper_audio_states(cfg, windows, seed + 100)[:1]
        sp = synth.whisper_special_tokens(eot)
        z = np.load(os.path.join(HERE, f"whisper_dec_{case}.npz"))
        texts = {"greedy": [int(t) for t in z["greedy_00_tokens"] if t < eot]}
        if "prompt9" in z.files:
            texts["extra"] = [int(t) for t in z["prompt9"] if t < eot]
        out = {}
        for name, text in texts.items():
            out[name + "_text"] = np.array(text, dtype=np.int32)
            if not text:
                out[name + "_probs64"], out[name + "_err32"] = np.zeros(0), np.float64(0.0)
                continue
            tokens = torch.tensor([[sp["<|startoftranscript|>"], sp["<|notimestamps|>"]] + text + [eot]])
            _, l64 = logits_of(dec64, emb, tokens, xa.double())
            _, l32 = logits_of(dec32, emb.float(), tokens, xa)
            ids = torch.tensor(text)[:, None]
            s64, s32 = l64[0, 1:1 + len(text), :eot].softmax(-1), l32[0, 1:1 + len(text), :eot].softmax(-1)
            p64 = s64.gather(1, ids)[:, 0]
            err = float((s32.double() - s64).abs().max())         # of the softmax rows the probabilities are taken from, as err32 of
            #                                                       whisper_dec_*.npz is of whole rows of logits
            print(f"{case} {name}: {len(text)} text tokens, probabilities {float(p64.min()):.3e} .. {float(p64.max()):.3e}, fp32 CPU error {err:.3e}")
            out[name + "_probs64"], out[name + "_err32"] = p64.numpy(), np.float64(err)
        path = os.path.join(HERE, f"whisper_align_{case}.npz")
        np.savez_compressed(path, **out)
        print(f"  wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
