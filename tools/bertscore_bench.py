#!/usr/bin/env python3
"""Throughput of BERTScore on caption-like input: roberta-large's shapes (synthetic weights, 24 layers cut after 17), pairs of
short sentences given as token-id rows.  Reports pairs/s of a whole ``BERTScorer.score_device`` call and the split between the
encoder and the matching launch (a second set of runs, synchronised between the two stages), each as the median with the
min .. max spread over the repeats.

    python tools/bertscore_bench.py [--pairs 2000] [--min-len 8] [--max-len 24] [--repeats 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hirest_amd import synth  # noqa: E402
from hirest_amd.bert_score import BERTScorer, DEFAULT_LAYERS  # noqa: E402


def spread(xs, scale=1e3, unit="ms"):
    return f"{statistics.median(xs) * scale:.2f} {unit} ({min(xs) * scale:.2f} .. {max(xs) * scale:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--min-len", type=int, default=8)
    ap.add_argument("--max-len", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    cfg = synth.ROBERTA_LARGE
    layers = DEFAULT_LAYERS[("roberta", cfg["num_hidden_layers"])]
    dev = torch.device("cuda:0")
    scorer = BERTScorer(config=cfg, state_dict=synth.roberta_state_dict(cfg, 71, layers), device=dev)
    assert scorer.num_layers == layers == 17
    # lengths count the two specials, as the issue's "8 - 24-token sentences"
    rows = synth.sentence_ids("bertscore_bench", 2 * a.pairs, 7, cfg["vocab_size"], a.min_len, a.max_len, cls_id=0, sep_id=2)
    cands, refs = rows[:a.pairs], rows[a.pairs:]
    for _ in range(a.warmup):
        scorer.score_device(cands, refs)
    torch.cuda.synchronize()
    total, enc, match, tok = [], [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        scorer.score_device(cands, refs)
        torch.cuda.synchronize()
        total.append(time.perf_counter() - t0)
    st = {}
    for _ in range(a.repeats):
        st = {}
        scorer.score_device(cands, refs, stats=st)
        enc.append(st["encoder_s"]); match.append(st["match_s"]); tok.append(st["tokenize_s"])
    print(f"{a.pairs} pairs, {st['unique_sentences']} unique sentences, {st['tokens']} tokens "
          f"(lengths {min(map(len, rows))} .. {max(map(len, rows))}), roberta-large widths, {layers} layers, {a.repeats} repeats after {a.warmup} warm-up")
    print(f"whole call      {spread(total)}  = {a.pairs / statistics.median(total):.0f} pairs/s")
    print(f"  host dedup    {spread(tok)}")
    print(f"  encoder       {spread(enc)}")
    print(f"  matching      {spread(match)}   (one hirest_bertscore_greedy launch, upload of its tables included)")
    print(json.dumps({"pairs": a.pairs, "tokens": st["tokens"], "pairs_per_s": a.pairs / statistics.median(total),
                      "total_ms": [round(x * 1e3, 3) for x in total], "encoder_ms": [round(x * 1e3, 3) for x in enc],
                      "match_ms": [round(x * 1e3, 3) for x in match]}))


if __name__ == "__main__":
    main()
