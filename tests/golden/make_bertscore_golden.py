#!/usr/bin/env python3
"""Generate the BERTScore fixtures: bytebpe.json, bertscore_tiny.npz, bertscore_wide.npz.  CPU only; needs the installed
``transformers`` and ``tokenizers`` (third party) and nothing of the reference tree.

``bert_score`` itself is not installed, so its pipeline is driven by hand from its published definition: the installed
``tokenizers`` ByteLevel + BPE pipeline (what ``RobertaTokenizerFast`` runs), ``transformers.RobertaModel`` with the seeded weights
of ``hirest_amd.synth`` and its layers after ``num_layers`` removed, then the library's padded greedy matching.  Stored figures:

* fp64 P, R, F per pair, computed pair by pair over the real tokens only (tests/_bertscore_ref.py);
* ``dev32``: the largest deviation from those of the library-form computation in fp32 (one padded batch, ``sim`` multiplied by the
  mask) with the same model: what two fp32 roundings of this arithmetic differ by, the unit of the GPU test's bar.

The library form in fp64 must agree with the per-pair form to 1e-12, and no row or column maximum may be <= 0 (only then could
the pad zeros of the library form win a maximum): both are asserted, the script fails otherwise.

    python tests/golden/make_bertscore_golden.py [bytebpe] [tiny] [wide]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _bertscore_ref as ref  # noqa: E402
from hirest_amd import synth  # noqa: E402

VOCAB_SIZE = 600
SPECIALS = ["<s>", "<pad>", "</s>", "<unk>", "<mask>"]        # roberta's ids 0 .. 3, <mask> after them

# ordinary tokens per sentence (without <s> </s>): candidate against reference, then one pair of the same sentence twice
TINY_CAND = [0, 1, 5, 9, 17, 30, 62, 3, 12, 7]
TINY_REF = [4, 1, 5, 0, 20, 33, 64, 64, 2, 7]
TINY_LAYERS, TINY_SEED = 3, 61
WIDE_CAND = [510, 0, 7, 23, 40, 100, 15, 31]
WIDE_REF = [12, 9, 30, 23, 33, 64, 200, 32]
WIDE_LAYERS, WIDE_SEED = 2, 62


def texts():
    with open(os.path.join(HERE, "wordpiece.json"), encoding="utf-8") as f:
        return json.load(f)["texts"]             # WORDPIECE_TEXTS (the edge strings) + the first 60 prompts


def hf_tokenizer(vocab, merges):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[tuple(m.split(" ")) for m in merges]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    tok.post_processor = processors.RobertaProcessing(sep=("</s>", vocab["</s>"]), cls=("<s>", vocab["<s>"]), trim_offsets=True,
                                                      add_prefix_space=False)
    return tok


def encode(tok, text, max_length):
    tok.enable_truncation(max_length=max_length)
    return tok.encode(text).ids


def gen_bytebpe():
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    trainer = trainers.BpeTrainer(vocab_size=VOCAB_SIZE, special_tokens=SPECIALS, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tok.train_from_iterator(texts(), trainer)
    d = tempfile.mkdtemp()
    tok.model.save(d)
    with open(os.path.join(d, "vocab.json"), encoding="utf-8") as f:
        vocab = json.load(f)
    with open(os.path.join(d, "merges.txt"), encoding="utf-8") as f:
        merges = [m for m in f.read().split("\n") if m and not m.startswith("#version")]
    assert [vocab[s] for s in SPECIALS] == [0, 1, 2, 3, 4] and len(vocab) <= VOCAB_SIZE
    hf = hf_tokenizer(vocab, merges)
    tt = texts()
    out = {"vocab": vocab, "merges": merges, "texts": tt, "ids": [encode(hf, t, 512) for t in tt],
           "ids_max8": [encode(hf, t, 8) for t in tt], "tokenizers": __import__("tokenizers").__version__}
    assert out["ids"][0] == [0, 2]
    with open(os.path.join(HERE, "bytebpe.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=True)
    print("wrote bytebpe.json", len(tt), "texts", len(vocab), "vocab entries", len(merges), "merges")


def load_model(cfg, seed, num_layers, dtype):
    from transformers import RobertaConfig, RobertaModel
    model = RobertaModel(RobertaConfig(**cfg, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0),
                         add_pooling_layer=False).eval()
    sd = {k[len("roberta."):]: v for k, v in synth.roberta_state_dict(cfg, seed).items()}
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k or "token_type_ids" in k for k in missing.missing_keys), missing
    model.encoder.layer = torch.nn.ModuleList(list(model.encoder.layer)[:num_layers])     # bert_score: the later layers are removed
    return model.to(dtype)


def padded_states(model, rows, pad_id):
    """one padded batch with its attention mask, as the library encodes -> [n, L, D] states and the [n, L] mask"""
    L = max(len(r) for r in rows)
    ids = torch.full((len(rows), L), pad_id, dtype=torch.int64)
    mask = torch.zeros((len(rows), L), dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r)
        mask[i, :len(r)] = 1
    with torch.no_grad():
        return model(input_ids=ids, attention_mask=mask).last_hidden_state, mask


def library_form(states, mask, cand, refi, rows, special_ids):
    """bert_score's greedy_cos_idf on padded batches (idf=False: weight 0 for the <s> / </s> ids, 1 elsewhere)"""
    hyp, hm = states[cand], mask[cand]
    rf, rm = states[refi], mask[refi]
    ids = torch.zeros(mask.shape, dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r)
    w = (mask.bool() & ~torch.isin(ids, torch.tensor(special_ids))).to(states.dtype)
    hyp = hyp / hyp.norm(dim=-1, keepdim=True)
    rf = rf / rf.norm(dim=-1, keepdim=True)
    sim = torch.bmm(hyp, rf.transpose(1, 2))
    sim = sim * torch.bmm(hm.unsqueeze(2).to(sim.dtype), rm.unsqueeze(1).to(sim.dtype))
    wp, wr = sim.max(dim=2)[0], sim.max(dim=1)[0]
    hw, rw = w[cand], w[refi]
    P = (wp * (hw / hw.sum(1, keepdim=True))).sum(1)
    R = (wr * (rw / rw.sum(1, keepdim=True))).sum(1)
    F = 2 * P * R / (P + R)
    P = P.masked_fill(hm.sum(1).eq(2), 0.0)
    R = R.masked_fill(rm.sum(1).eq(2), 0.0)
    F = F.masked_fill(torch.isnan(F), 0.0)
    return torch.stack([P, R, F], 1)


def reference_numbers(cfg, seed, num_layers, rows, cand, refi):
    """-> (packed fp32 states of the fp64 model, offsets, fp64 [n_pairs, 3], dev32)"""
    pad = cfg["pad_token_id"]
    m64 = load_model(cfg, seed, num_layers, torch.float64)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    packed = np.zeros((int(off[-1]), cfg["hidden_size"]))
    for i, r in enumerate(rows):                  # every sentence on its own: no padding anywhere
        with torch.no_grad():
            packed[off[i]:off[i + 1]] = m64(input_ids=torch.tensor([r])).last_hidden_state[0].numpy()
    w = ref.special_weights(off)
    triples, lowest = [], np.inf
    for a, b in zip(cand, refi):
        sa, sb = slice(off[a], off[a + 1]), slice(off[b], off[b + 1])
        P, R, F, lo = ref.pair_scores(packed[sa], packed[sb], w[sa], w[sb])
        triples.append((P, R, F))
        lowest = min(lowest, lo)
    triples = np.asarray(triples)
    assert lowest > 0, f"a row or column maximum is {lowest} <= 0: the library's pad zeros would win it; change the inputs"
    st, mask = padded_states(m64, rows, pad)
    lib64 = library_form(st, mask, cand, refi, rows, [cfg["bos_token_id"], cfg["eos_token_id"]]).numpy()
    assert np.abs(lib64 - triples).max() <= 1e-12, np.abs(lib64 - triples).max()
    st, mask = padded_states(load_model(cfg, seed, num_layers, torch.float32), rows, pad)
    lib32 = library_form(st, mask, cand, refi, rows, [cfg["bos_token_id"], cfg["eos_token_id"]]).double().numpy()
    dev32 = float(np.abs(lib32 - triples).max())
    print(f"  lowest maximum {lowest:.4f}  padded fp64 vs per pair {np.abs(lib64 - triples).max():.2e}  dev32 {dev32:.3e}")
    return packed.astype(np.float32), off, triples, dev32


def sentence_of(hf, words, n, start):
    """a sentence of exactly n ordinary tokens, built word by word from the prompts"""
    if n == 0:
        return "  "
    text, k = "", start
    for _ in range(10 * len(words)):
        cand = (text + " " + words[k % len(words)]).strip()
        k += 1
        m = len(hf.encode(cand).ids) - 2
        if m <= n:
            text = cand
        if m == n:
            return text
    raise RuntimeError(f"no sentence of {n} tokens found")


def gen_tiny():
    with open(os.path.join(HERE, "bytebpe.json"), encoding="utf-8") as f:
        bpe = json.load(f)
    with open(os.path.join(HERE, "test_prompts.json"), encoding="utf-8") as f:
        words = [w for p in json.load(f)[60:200] for w in p.lower().split()]
    cfg = synth.ROBERTA_TINY
    hf = hf_tokenizer(bpe["vocab"], bpe["merges"])
    hf.enable_truncation(max_length=cfg["max_position_embeddings"] - cfg["pad_token_id"] - 1)
    sents = [sentence_of(hf, words, n, 37 * i) for i, n in enumerate(TINY_CAND + TINY_REF)]
    sents.append("Whisk the eggs, then add the flour!")
    rows = [hf.encode(s.strip()).ids for s in sents]
    assert [len(r) - 2 for r in rows[:-1]] == TINY_CAND + TINY_REF and max(map(max, rows)) < cfg["vocab_size"]
    n = len(TINY_CAND)
    cand = list(range(n)) + [2 * n]
    refi = list(range(n, 2 * n)) + [2 * n]
    states, off, triples, dev32 = reference_numbers(cfg, TINY_SEED, TINY_LAYERS, rows, cand, refi)
    np.savez_compressed(os.path.join(HERE, "bertscore_tiny.npz"), ids=np.concatenate([np.asarray(r, np.int64) for r in rows]),
                        lens=np.asarray([len(r) for r in rows], np.int64), cand=np.asarray(cand, np.int64),
                        ref=np.asarray(refi, np.int64), states=states, triples=triples, dev32=dev32, seed=TINY_SEED,
                        num_layers=TINY_LAYERS, texts=np.asarray(sents))
    print("wrote bertscore_tiny.npz", len(rows), "sentences", len(cand), "pairs")
    print(triples)


def gen_wide():
    cfg = synth.ROBERTA_WIDE
    lens = WIDE_CAND + WIDE_REF
    rows = [synth.sentence_ids(f"bertscore.wide.{i}", 1, WIDE_SEED, cfg["vocab_size"], L + 2, L + 2, cls_id=0, sep_id=2)[0]
            for i, L in enumerate(lens)]
    assert [len(r) - 2 for r in rows] == lens
    n = len(WIDE_CAND)
    cand, refi = list(range(n)), list(range(n, 2 * n))
    _, _, triples, dev32 = reference_numbers(cfg, WIDE_SEED, WIDE_LAYERS, rows, cand, refi)
    np.savez_compressed(os.path.join(HERE, "bertscore_wide.npz"), ids=np.concatenate([np.asarray(r, np.int64) for r in rows]),
                        lens=np.asarray([len(r) for r in rows], np.int64), cand=np.asarray(cand, np.int64),
                        ref=np.asarray(refi, np.int64), triples=triples, dev32=dev32, seed=WIDE_SEED, num_layers=WIDE_LAYERS)
    print("wrote bertscore_wide.npz", len(rows), "sentences", n, "pairs")
    print(triples)


if __name__ == "__main__":
    jobs = {"bytebpe": gen_bytebpe, "tiny": gen_tiny, "wide": gen_wide}
    for name in (sys.argv[1:] or list(jobs)):
        jobs[name]()
