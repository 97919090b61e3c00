"""GPT-2 / RoBERTa byte-level BPE from ``vocab.json`` + ``merges.txt``: the tokenizer of roberta-large, which ``bert_score`` uses
for ``lang='en'`` (evaluate.py:294-297).

The published algorithm, restated: the text is cut by the GPT-2 pre-tokenisation pattern (no prefix space is added), each piece's
UTF-8 bytes are written in the printable bytes-to-unicode alphabet, and inside a piece the adjacent pair with the lowest merge rank
is merged until no listed pair is left; the pieces' symbols are looked up in the vocabulary.  ``encode`` wraps them in ``<s>`` /
``</s>`` and truncates with the two specials included.  Pinned id for id to the ``tokenizers`` ByteLevel + BPE pipeline, which is
what ``RobertaTokenizerFast`` runs (tests/golden/bytebpe.json).  Integer work on the CPU.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterable, List, Sequence, Tuple, Union

import regex

PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"


def bytes_to_unicode() -> Dict[int, str]:
    """Byte -> printable character: the printable Latin-1 bytes stand for themselves, the other 68 are moved to U+0100 onwards."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    table, n = {b: chr(b) for b in keep}, 0
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + n)
            n += 1
    return table


class ByteBPETokenizer:
    def __init__(self, vocab: Dict[str, int], merges: Iterable[Union[str, Sequence[str]]], bos_token: str = "<s>",
                 eos_token: str = "</s>", pad_token: str = "<pad>", unk_token: str = "<unk>"):
        """``vocab``: symbol -> id (``vocab.json``); ``merges``: the lines of ``merges.txt`` ("a b") or pairs, in rank order (a
        ``#version`` header line and blank lines are skipped)."""
        self.vocab = {str(k): int(v) for k, v in vocab.items()}
        self.ranks: Dict[Tuple[str, str], int] = {}
        for m in merges:
            if isinstance(m, str):
                m = m.rstrip("\n")
                if not m or m.startswith("#version"):
                    continue
                m = m.split(" ")
            if len(m) != 2:
                raise ValueError(f"malformed merge {m!r}")
            self.ranks.setdefault((m[0], m[1]), len(self.ranks))
        for name, tok in (("bos", bos_token), ("eos", eos_token), ("pad", pad_token)):
            if tok not in self.vocab:
                raise ValueError(f"the vocabulary has no {tok!r}")
            setattr(self, name + "_id", self.vocab[tok])
        self.unk_id = self.vocab.get(unk_token)
        self.cls_id, self.sep_id = self.bos_id, self.eos_id
        self._byte = bytes_to_unicode()
        self._split = regex.compile(PATTERN)
        self._cache: Dict[str, List[int]] = {}

    @classmethod
    def from_dir(cls, model_dir: str, **kw) -> "ByteBPETokenizer":
        with open(os.path.join(model_dir, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(model_dir, "merges.txt"), encoding="utf-8") as f:
            merges = f.read().split("\n")
        return cls(vocab, merges, **kw)

    def _bpe(self, piece: str) -> List[int]:
        """one pre-token (already in the byte alphabet) -> ids"""
        hit = self._cache.get(piece)
        if hit is not None:
            return hit
        word = list(piece)
        while len(word) > 1:
            best, at = None, -1
            for i in range(len(word) - 1):
                r = self.ranks.get((word[i], word[i + 1]))
                if r is not None and (best is None or r < best):
                    best, at = r, i
            if best is None:
                break
            a, b = word[at], word[at + 1]
            out, i = [], 0
            while i < len(word):                      # every occurrence of the pair, left to right
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = out
        ids = []
        for sym in word:
            i = self.vocab.get(sym, self.unk_id)
            if i is None:
                raise KeyError(f"symbol {sym!r} is not in the vocabulary and it has no unknown token")
            ids.append(i)
        self._cache[piece] = ids
        return ids

    def tokenize_ids(self, text: str) -> List[int]:
        """ids without ``<s>`` / ``</s>``"""
        ids: List[int] = []
        for piece in self._split.findall(text):
            ids.extend(self._bpe("".join(self._byte[b] for b in piece.encode("utf-8"))))
        return ids

    def encode(self, text: str, max_seq_length: int = 512) -> List[int]:
        ids = self.tokenize_ids(text)[: max(max_seq_length - 2, 0)]
        return [self.bos_id] + ids + [self.eos_id]

    def encode_batch(self, texts: Sequence[str], max_seq_length: int = 512) -> List[List[int]]:
        return [self.encode(t, max_seq_length) for t in texts]

    def decode(self, ids: Iterable[int]) -> str:
        """ids -> text: the symbols' characters mapped back to bytes, decoded as UTF-8 (malformed sequences become U+FFFD).  Ids without
        a symbol raise KeyError."""
        if not hasattr(self, "_sym"):
            self._sym = {i: s for s, i in self.vocab.items()}
            self._unbyte = {c: b for b, c in self._byte.items()}
        chars = "".join(self._sym[int(i)] for i in ids)
        return bytes(self._unbyte[c] for c in chars).decode("utf-8", errors="replace")
