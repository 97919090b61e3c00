#!/usr/bin/env python
"""Every ``.wav`` of a directory -> an ``.srt`` beside its name, with ``hirest_amd.whisper``: the arguments and the option block of the
reference's ``extraction/whisper_ASR/extract_ASR.py``, our own code against our own API.

    python tools/extract_asr.py --model /models/whisper-small.en --audio_dir data/audio --asr_dir data/ASR

``--model`` is a local OpenAI ``.pt`` checkpoint or a Hugging Face model directory, never a model name: nothing is downloaded.
``--tokenizer`` is a directory with ``vocab.json`` and ``merges.txt`` (default: the model directory).
``--language`` is a language's name or code (default English, as the reference's), or ``auto`` / ``"Auto detection"``: a multilingual
model then detects each file's language on its first 30 seconds.  ``--task translate`` writes English subtitles for any language.
``--word_timestamps`` also writes ``<name>.json`` beside each ``.srt``: the segments with their words (``word``, ``start``, ``end``,
``probability``); the ``.srt`` is what it is without the option.
``--precision bf16x3`` runs the audio encoder's blocks on split bf16 operands (the reference runs them at fp16); without
it the environment's ``HIREST_WHISPER_PRECISION`` decides, else fp32.
``--graph`` replays every decoding loop's iterations from a captured hipGraph: the same subtitles, fewer launches on
the host; without it the environment's ``HIREST_WHISPER_GRAPH`` decides, else off.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hirest_amd import whisper  # noqa: E402


def language_argument(value: str):
    """``--language``: "auto" / "Auto detection" (the reference's menu entry) -> None, anything else -> its language code"""
    if value.strip().lower() in ("auto", "auto detection"):
        return None
    try:
        return whisper.language_code(value)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", type=str, required=True, help="local .pt checkpoint or Hugging Face model directory")
    ap.add_argument("--audio_dir", type=str, required=True)
    ap.add_argument("--asr_dir", type=str, required=True)
    ap.add_argument("--tokenizer", type=str, default=None, help="directory with vocab.json and merges.txt (default: --model)")
    ap.add_argument("--language", type=language_argument, default="en",
                    help="a language's name or code, or 'auto' / 'Auto detection' (multilingual models: detected per file); default English")
    ap.add_argument("--task", type=str, default="transcribe", choices=["transcribe", "translate"])
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--files_in_flight", type=int, default=whisper.FILES_IN_FLIGHT,
                    help="files whose current windows are decoded together (whisper.transcribe_many); 1: one file at a time (whisper.transcribe)")
    ap.add_argument("--word_timestamps", action="store_true", help="align every window's words (whisper.timing) and write <name>.json")
    ap.add_argument("--precision", type=str, default=None, choices=list(whisper.AudioEncoder.PRECISIONS),
                    help="the audio encoder's precision (default: HIREST_WHISPER_PRECISION, else fp32); the decoder is exact fp32 always")
    ap.add_argument("--graph", action="store_true",
                    help="replay the decoding loop from a captured hipGraph (default: HIREST_WHISPER_GRAPH, else off); the same output")
    args = ap.parse_args(argv)
    if args.files_in_flight < 1:
        ap.error("--files_in_flight must be at least 1")
    print(args)

    model = whisper.load_model(args.model, args.device, tokenizer=args.tokenizer, precision=args.precision).eval()
    print("Model loaded: ", args.model, "at device", model.device, "encoder precision", model.precision)

    # the reference's option block.  Its first temperature is 0.15, so every window is sampled (best_of candidates) and the beam options
    # are never used: transcribe() drops them above temperature 0.
    temperature, temperature_increment_on_fallback = 0.15, 0.2
    options = dict(language=args.language, task=args.task, best_of=5, beam_size=5, patience=1.0, length_penalty=None, suppress_tokens="-1",
                   initial_prompt=None, condition_on_previous_text=True, fp16=True, compression_ratio_threshold=2.4, logprob_threshold=-1.0,
                   no_speech_threshold=0.6, seed=args.seed, word_timestamps=args.word_timestamps)
    temperatures = tuple(np.arange(temperature, 1.0 + 1e-6, temperature_increment_on_fallback))
    if args.graph:
        options["graph"] = True

    out_dir = Path(args.asr_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    wavs = sorted(Path(args.audio_dir).glob("*.wav"))
    if args.files_in_flight > 1:                                      # the current windows of that many files share one decoding loop
        results = whisper.transcribe_many(model, [str(w) for w in wavs], files_in_flight=args.files_in_flight, temperature=temperatures, **options)
    else:
        results = (whisper.transcribe(model, str(wav), temperature=temperatures, **options) for wav in wavs)
    for wav, result in zip(wavs, results):
        with open(out_dir / (wav.stem + ".srt"), "w", encoding="utf-8") as f:
            whisper.utils.write_srt(result["segments"], file=f)
        if args.word_timestamps:
            keep = ("id", "seek", "start", "end", "text", "words")
            with open(out_dir / (wav.stem + ".json"), "w", encoding="utf-8") as f:
                json.dump({"language": result["language"], "segments": [{k: s[k] for k in keep} for s in result["segments"]]}, f,
                          ensure_ascii=False, indent=1)
        print(f"{wav.name}: {len(result['segments'])} segments")


if __name__ == "__main__":
    main()
