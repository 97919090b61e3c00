"""BERTScore of step captions on MI355X: the ``bert_score`` call of evaluate_moment_summarization (evaluate.py:294-297)::

    from hirest_amd.bert_score import score
    p, r, f = score(cands, refs, model_type="/models/roberta-large", lang='en', verbose=True, device=f"cuda:{gpu_device}")
    ... "BERTScore_F1": f.mean().item()

``bert_score`` is not under the reference tree; the algorithm is restated from its published definition and pinned with synthetic
weights against ``transformers.RobertaModel`` (tests/golden/bertscore_*.npz).  Per (candidate, reference) pair:

1. each sentence is stripped and tokenized to ``<s> tokens </s>`` (an empty sentence: the two specials), truncated to the model's
   maximum length with the specials included (roberta: ``max_position_embeddings - pad_token_id - 1`` = 512);
2. token states = the encoder's output after its first ``num_layers`` layers (``lang='en'`` = roberta-large, 17 of 24), later layers
   removed, pooler unused, token type 0, RoBERTa position of token i = ``pad_token_id + 1 + i``;
3. every state is divided by its L2 norm; ``sim[i][j] = <c_i, r_j>`` over all tokens of both sentences, specials included;
4. ``wp[i] = max_j sim[i][j]``, ``wr[j] = max_i sim[i][j]``; with weight 1 for ordinary tokens and 0 for the first and last
   (``idf=False``), ``P = sum_i w_i wp[i] / sum_i w_i``, R likewise over the reference, ``F = 2PR / (P + R)``.  A sentence without an
   ordinary token has weight sum 0: its P (candidate) or R (reference) is 0 and a NaN F becomes 0.

Device side: every unique sentence is encoded once by the exact-fp32 packed encoder of ``sentence_encoder`` (no padding rows), and
one ``hirest_bertscore_greedy`` launch scores all pairs (fp32 MFMA cosines, maxima from the accumulators, ``sim`` never stored).

One deliberate difference from the library: it pads a batch and multiplies ``sim`` by the mask, so pad positions enter each maximum
as 0 and a result depends on what else is in the batch whenever every real cosine of some row or column is negative.  Here no pad
rows exist and a maximum is over the pair's real tokens only; the two agree unless such an all-negative row or column occurs.

Not built (each raises NotImplementedError under its name): ``idf=True``, ``rescale_with_baseline``, ``all_layers``, several
references per candidate.  There is no CPU path: off-GPU ``score`` raises.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .sentence_encoder import PackedBertEncoder, _load_weights

# (architecture, depth) -> the layer bert_score takes the states from
DEFAULT_LAYERS = {("roberta", 24): 17, ("roberta", 12): 10, ("roberta", 6): 5, ("bert", 12): 9, ("bert", 24): 18}
LANG_MODEL = {"en": "roberta-large"}


class _TokenEncoder(PackedBertEncoder):
    _NAME = "hirest_amd.BERTScorer"

    def __init__(self, config, state_dict, num_layers):
        super().__init__()
        self._init_encoder(config, state_dict, num_layers)


class BERTScorer:
    def __init__(self, model_type: Optional[str] = None, num_layers: Optional[int] = None, lang: Optional[str] = None, idf: bool = False,
                 device: Optional[Union[str, torch.device]] = None, *, config: Optional[dict] = None,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, vocab=None, merges=None, all_layers: bool = False,
                 rescale_with_baseline: bool = False):
        """``model_type``: a local Hugging Face model directory (``config.json``, ``model.safetensors`` or ``pytorch_model.bin``, and
        ``vocab.json`` + ``merges.txt`` for RoBERTa or ``vocab.txt`` for BERT) — a hub name cannot be downloaded, so a name that is
        not a directory raises — or explicit ``config`` + ``state_dict`` (+ ``vocab`` and, for RoBERTa, ``merges``).  ``num_layers``
        defaults by architecture and depth (roberta 24 -> 17, 12 -> 10, 6 -> 5; bert 12 -> 9, 24 -> 18) and must be given otherwise."""
        if idf:
            raise NotImplementedError("idf=True is not built (only idf=False, evaluate.py:295)")
        if all_layers:
            raise NotImplementedError("all_layers is not built")
        if rescale_with_baseline:
            raise NotImplementedError("rescale_with_baseline is not built")
        if config is None:
            if model_type is None and lang is not None:
                if lang not in LANG_MODEL:
                    raise NotImplementedError(f"lang={lang!r}: only {sorted(LANG_MODEL)} has a default model")
                model_type = LANG_MODEL[lang]
            if model_type is None:
                raise ValueError("either lang or model_type (a local model directory) is needed")
            if not os.path.isdir(model_type):
                raise FileNotFoundError(f"{model_type!r} is not a local model directory (no network access: download "
                                        f"{model_type} beforehand and pass its path)")
            with open(os.path.join(model_type, "config.json")) as f:
                config = json.load(f)
            state_dict = _load_weights(model_type)
            if vocab is None:
                vocab, merges = self._read_vocab(model_type, config)
        arch = "roberta" if config.get("model_type") == "roberta" else "bert"
        if num_layers is None:
            num_layers = DEFAULT_LAYERS.get((arch, int(config["num_hidden_layers"])))
            if num_layers is None:
                raise ValueError(f"no default num_layers for a {arch} of {config['num_hidden_layers']} layers: pass num_layers")
        self.model_type, self.arch, self.num_layers, self.idf = model_type, arch, int(num_layers), False
        self.encoder = _TokenEncoder(config, state_dict, self.num_layers)
        self.max_length = int(config["max_position_embeddings"]) - self.encoder.pos_offset
        self.tokenizer = self._make_tokenizer(arch, vocab, merges)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.encoder.to(device)

    @staticmethod
    def _read_vocab(model_dir: str, config: dict):
        if config.get("model_type") == "roberta":
            with open(os.path.join(model_dir, "vocab.json"), encoding="utf-8") as f:
                vocab = json.load(f)
            with open(os.path.join(model_dir, "merges.txt"), encoding="utf-8") as f:
                return vocab, f.read().split("\n")
        with open(os.path.join(model_dir, "vocab.txt"), encoding="utf-8") as f:
            return f.readlines(), None

    @staticmethod
    def _make_tokenizer(arch: str, vocab, merges):
        if vocab is None:
            return None
        if arch == "roberta":
            from .bytebpe import ByteBPETokenizer
            if merges is None:
                raise ValueError("a RoBERTa vocabulary needs its merges")
            return ByteBPETokenizer(vocab, merges)
        from .wordpiece import WordPieceTokenizer
        return WordPieceTokenizer(vocab)

    @property
    def device(self) -> torch.device:
        return self.encoder.device

    def to(self, device) -> "BERTScorer":
        self.encoder.to(device)
        return self

    def tokenize(self, sentence: str) -> List[int]:
        if self.tokenizer is None:
            raise RuntimeError("no vocabulary was given: pass token-id rows instead of strings")
        return self.tokenizer.encode(str(sentence).strip(), self.max_length)

    def _rows(self, sentences: Sequence) -> Tuple[List[Tuple[int, ...]], List[int]]:
        """sentences (strings, or token-id rows with their two specials) -> the unique id rows in order of first use, and each
        sentence's index among them"""
        uniq: Dict[Tuple[int, ...], int] = {}
        of_text: Dict[str, int] = {}
        index = []
        for s in sentences:
            if isinstance(s, str):
                if s not in of_text:
                    of_text[s] = uniq.setdefault(tuple(self.tokenize(s)), len(uniq))
                index.append(of_text[s])
            elif len(s) and isinstance(s[0], str):
                raise NotImplementedError("several references per candidate are not built")
            else:
                row = tuple(int(t) for t in s)
                if not 2 <= len(row) <= self.max_length:
                    raise ValueError(f"a token-id row has {len(row)} ids (2 .. {self.max_length}, specials included)")
                index.append(uniq.setdefault(row, len(uniq)))
        return list(uniq), index

    @torch.no_grad()
    def token_states(self, rows: Sequence[Sequence[int]]) -> Tuple[torch.Tensor, np.ndarray]:
        """token-id rows -> ([tokens, hidden] fp32 states on the device, packed row after row; int64 [n + 1] row offsets)"""
        enc = self.encoder
        dev = enc.device
        if dev.type != "cuda":
            raise RuntimeError("hirest_amd.BERTScorer runs on MI355X only (no CPU fallback); move the scorer to a GPU")
        off = np.zeros(len(rows) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        states = torch.empty((int(off[-1]), enc.hidden), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for s, e, ids, pos_ids, seq_off, max_len in enc._passes(rows):
                states[off[s]:off[e]] = enc._token_states(ids, pos_ids, seq_off, e - s, max_len)
        return states, off

    @torch.no_grad()
    def score_device(self, cands: Sequence, refs: Sequence, stats: Optional[dict] = None) -> torch.Tensor:
        """[len(cands), 3] fp32 (P, R, F) on the device: every unique sentence encoded once, one scoring launch for all pairs.
        ``stats`` (a dict): filled with counts and the seconds of the encoder and of the matching launch (each then synchronised)."""
        import time
        if len(cands) != len(refs):
            raise ValueError(f"{len(cands)} candidates against {len(refs)} references")
        dev = self.encoder.device
        if dev.type != "cuda":
            raise RuntimeError("hirest_amd.BERTScorer runs on MI355X only (no CPU fallback); move the scorer to a GPU")
        if not len(cands):
            return torch.empty((0, 3), dtype=torch.float32, device=dev)
        t0 = time.perf_counter()
        rows, index = self._rows(list(cands) + list(refs))
        t1 = time.perf_counter()
        states, off = self.token_states(rows)
        if stats is not None:
            torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        w = np.ones(int(off[-1]), np.float32)                      # idf=False: 1, and 0 for a sentence's first and last token
        w[off[:-1]] = 0.0
        w[off[1:] - 1] = 0.0
        out = ops.bertscore_greedy(states, torch.from_numpy(off), torch.from_numpy(w).to(dev),
                                   torch.tensor(index[:len(cands)], dtype=torch.int32), torch.tensor(index[len(cands):], dtype=torch.int32))
        if stats is not None:
            torch.cuda.synchronize(dev)
            stats.update(pairs=len(cands), unique_sentences=len(rows), tokens=int(off[-1]), tokenize_s=t1 - t0, encoder_s=t2 - t1,
                         match_s=time.perf_counter() - t2)
        return out

    def score(self, cands: Sequence, refs: Sequence, verbose: bool = False, batch_size: int = 64, return_hash: bool = False):
        """``(P, R, F)``: three fp32 CPU tensors of ``len(cands)``, rows in input order.  ``cands`` / ``refs``: strings, or token-id
        rows that already carry their two specials.  ``verbose`` and ``batch_size`` have no effect on the numbers."""
        if return_hash:
            raise NotImplementedError("return_hash is not built")
        out = self.score_device(cands, refs).cpu()
        return out[:, 0].contiguous(), out[:, 1].contiguous(), out[:, 2].contiguous()


def score(cands, refs, model_type: Optional[str] = None, num_layers: Optional[int] = None, verbose: bool = False, idf: bool = False,
          device=None, batch_size: int = 64, nthreads: int = 4, all_layers: bool = False, lang: Optional[str] = None,
          return_hash: bool = False, rescale_with_baseline: bool = False, baseline_path: Optional[str] = None, use_fast_tokenizer: bool = False):
    """``bert_score.score`` as evaluate.py:295 calls it; ``model_type`` must be a local model directory (with ``lang='en'`` alone the
    error names roberta-large).  ``batch_size``, ``verbose``, ``nthreads`` and ``use_fast_tokenizer`` are accepted and have no effect
    on the numbers."""
    if baseline_path is not None:
        raise NotImplementedError("baseline_path (rescale_with_baseline) is not built")
    if lang is None and model_type is None:
        raise ValueError("Either lang or model_type should be specified")
    scorer = BERTScorer(model_type=model_type, num_layers=num_layers, lang=lang, idf=idf, device=device, all_layers=all_layers,
                        rescale_with_baseline=rescale_with_baseline)
    return scorer.score(cands, refs, return_hash=return_hash)
