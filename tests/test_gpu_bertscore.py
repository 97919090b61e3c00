"""BERTScore on the device: the hirest_bertscore_greedy kernel against its fp64 restatement (tests/_bertscore_ref.py) at the tile
edges, its batch invariance, BERTScorer end to end against the fp64 transformers.RobertaModel fixtures
(tests/golden/bertscore_*.npz, written by make_bertscore_golden.py), evaluate_bert_score, and that the encoder code shared with
SentenceTransformer leaves its bits alone."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bertscore_ref as ref  # noqa: E402
from hirest_amd import bert_score, evaluation, ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = [4, 64, 68, 1024]
LENS = [2, 3, 31, 32, 33, 64, 65]          # the 32-row tile's edges on both axes; 2 = an empty sentence (the two specials)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _case(D):
    """Sentences 0..6: candidates of LENS, 7..13: references of LENS, 14: a 31-token sentence whose weights are all zero.
    Pairs: every candidate x reference length, each sentence against itself, repeats of earlier pairs, the zero-weight sentence on
    either side, and one pair with a sentence id out of range."""
    g = torch.Generator().manual_seed(1000 + D)
    lens = LENS + LENS + [31]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    # Token states of one model point roughly one way (every row and column maximum of the fixtures is > 0.28).  A common offset gives
    # the random rows that property: with P, R > 0 the slopes of F = 2PR / (P + R) obey (dF/dP + dF/dR) / 2 <= 1 and the bar on F
    # follows from the bar on P and R; near P + R = 0 it would not.
    states = torch.randn((int(off[-1]), D), generator=g, dtype=torch.float32) + 1.0
    w = ref.special_weights(off)
    w[off[4] + 1:off[5] - 1] = torch.rand(LENS[4] - 2, generator=g).numpy() + 0.5      # weights are an input: not only 0 / 1
    w[off[14]:off[15]] = 0
    n = len(LENS)
    cand = [i for i in range(n) for _ in range(n)] + list(range(2 * n)) + [3, 3, 5] + [14, 6, 14]
    refs = [n + j for _ in range(n) for j in range(n)] + list(range(2 * n)) + [n + 4, n + 4, 5] + [n + 2, 14, 14]
    bad = len(cand)
    cand.append(len(lens))                   # one id outside [0, n_seq)
    refs.append(0)
    want = ref.greedy(states.numpy(), off, w, cand, refs)
    assert np.nanmin(want[:, :2]) >= 0 and np.nanmin(want[:, :2][want[:, :2] != 0]) > 0.1      # a property of the inputs
    return {"D": D, "states": states, "off": off, "w": torch.from_numpy(w), "cand": cand, "ref": refs, "bad": bad, "want": want}


_CASES = {}


def case(D):                                # the fp64 reference of a width: computed once, shared, never modified
    if D not in _CASES:
        _CASES[D] = _case(D)
    return _CASES[D]


def run(c, dev, cand=None, refs=None):
    cand = c["cand"] if cand is None else cand
    refs = c["ref"] if refs is None else refs
    return ops.bertscore_greedy(c["states"].to(dev), torch.from_numpy(c["off"]), c["w"].to(dev), torch.tensor(cand), torch.tensor(refs)).cpu()


@pytest.mark.parametrize("D", DIMS)
def test_kernel_against_fp64(dev, D):
    """A length-D fp32 dot of unit vectors is within D 2^-24 of exact, P and R are convex combinations of such dots: (D + 8) 2^-24
    for P and R, twice that for F."""
    c = case(D)
    got = run(c, dev).double().numpy()
    want, bad = c["want"], c["bad"]
    assert np.isnan(got[bad]).all() and np.isnan(want[bad]).all()
    ok = np.arange(len(want)) != bad
    assert not np.isnan(got[ok]).any()                                    # NaN for that pair only
    err = np.abs(got[ok] - want[ok])
    bar = (D + 8) * 2.0 ** -24
    print(f"D={D}: max |P,R - fp64| = {err[:, :2].max():.3e} (bar {bar:.3e}), max |F - fp64| = {err[:, 2].max():.3e} (bar {2 * bar:.3e})")
    assert err[:, :2].max() <= bar
    assert err[:, 2].max() <= 2 * bar
    n = len(LENS)
    same = slice(n * n, n * n + 2 * n)                                    # cand == ref: P = R = 1 wherever a token has weight
    ordinary = np.array((LENS + LENS)) > 2
    assert np.abs(got[same][ordinary] - 1).max() <= 2 * bar
    assert (got[same][~ordinary] == 0).all()                              # an empty sentence against itself: the zero rules
    # repeats of a pair give the same bits; the zero-weight sentence has P (or R) = 0 and F = 0 exactly
    assert (got[n * n + 2 * n] == got[n * n + 2 * n + 1]).all() and (got[n * n + 2 * n] == got[3 * n + 4]).all()
    z = n * n + 2 * n + 3
    assert got[z, 0] == 0 and got[z, 2] == 0 and got[z, 1] > 0
    assert got[z + 1, 1] == 0 and got[z + 1, 2] == 0 and got[z + 1, 0] > 0
    assert (got[z + 2] == 0).all()
    # an empty candidate (row block 0) / reference (column 0): P / R exactly 0 and F exactly 0, the other side still computed
    assert (got[1:n, 0] == 0).all() and (got[1:n, 2] == 0).all() and (got[1:n, 1] != 0).all()
    assert (got[n:n * n:n, 1] == 0).all() and (got[n:n * n:n, 2] == 0).all()


@pytest.mark.parametrize("D", DIMS)
def test_batch_invariance(dev, D):
    c = case(D)
    full = run(c, dev)
    n = len(c["cand"])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7)).tolist()
    shuffled = run(c, dev, [c["cand"][i] for i in perm], [c["ref"][i] for i in perm])
    assert torch.equal(torch.nan_to_num(shuffled, nan=-7.0), torch.nan_to_num(full[perm], nan=-7.0))
    alone = torch.cat([run(c, dev, [c["cand"][i]], [c["ref"][i]]) for i in range(n)])
    assert torch.equal(torch.nan_to_num(alone, nan=-7.0), torch.nan_to_num(full, nan=-7.0))
    assert run(c, dev, [], []).shape == (0, 3)


def test_strided_rows(dev):
    """states with a row stride wider than D (a column slice of a wider matrix) give the bits of the packed copy"""
    c = case(68)
    wide = torch.zeros((c["states"].shape[0], 80), device=dev)
    wide[:, :68] = c["states"].to(dev)
    got = ops.bertscore_greedy(wide[:, :68], torch.from_numpy(c["off"]), c["w"].to(dev), torch.tensor(c["cand"]), torch.tensor(c["ref"])).cpu()
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(run(c, dev), nan=-7.0))


# ------------------------------------------------------------------------------------------------------------ end to end

def _fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    rows = [r.tolist() for r in np.split(g["ids"], np.cumsum(g["lens"])[:-1])]
    return g, rows


@pytest.fixture(scope="module")
def bpe():
    with open(os.path.join(GOLDEN, "bytebpe.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tiny_scorer(dev, bpe):
    g = np.load(os.path.join(GOLDEN, "bertscore_tiny.npz"))
    cfg, L = synth.ROBERTA_TINY, int(g["num_layers"])
    return bert_score.BERTScorer(config=cfg, state_dict=synth.roberta_state_dict(cfg, int(g["seed"]), L), num_layers=L,
                                 vocab=bpe["vocab"], merges=bpe["merges"], device=dev)


def _check(got, g, rows, what):
    """against the fp64 triples within 8 x dev32 (both sides are fp32 roundings of the same arithmetic and differ in summation
    order only; a wrongly matched token moves a score by orders of magnitude more); the zero rules exactly"""
    got = torch.stack(got, 1).double().numpy()
    err = np.abs(got - g["triples"]).max()
    print(f"{what}: max |P,R,F - fp64| = {err:.3e}, dev32 = {float(g['dev32']):.3e}, bar = {8 * float(g['dev32']):.3e}")
    assert err <= 8 * float(g["dev32"])
    for p, (a, b) in enumerate(zip(g["cand"], g["ref"])):
        if len(rows[a]) == 2:
            assert got[p, 0] == 0.0 and got[p, 2] == 0.0 and got[p, 1] > 0
        if len(rows[b]) == 2:
            assert got[p, 1] == 0.0 and got[p, 2] == 0.0 and got[p, 0] > 0


def test_tiny_end_to_end_from_ids_and_strings(dev, tiny_scorer):
    g, rows = _fixture("bertscore_tiny")
    P, R, F = tiny_scorer.score([rows[i] for i in g["cand"]], [rows[i] for i in g["ref"]])
    assert P.dtype == torch.float32 and P.device.type == "cpu" and P.shape == (len(g["cand"]),)
    _check((P, R, F), g, rows, "tiny, ids")
    texts = [str(t) for t in g["texts"]]
    S = tiny_scorer.score([texts[i] for i in g["cand"]], [texts[i] for i in g["ref"]])
    _check(S, g, rows, "tiny, strings")
    assert all(torch.equal(a, b) for a, b in zip(S, (P, R, F)))           # the same ids, the same bits


def test_wide_end_to_end_from_ids(dev):
    g, rows = _fixture("bertscore_wide")
    assert max(map(len, rows)) == 512 and min(map(len, rows)) == 2
    cfg, L = synth.ROBERTA_WIDE, int(g["num_layers"])
    scorer = bert_score.BERTScorer(config=cfg, state_dict=synth.roberta_state_dict(cfg, int(g["seed"]), L), num_layers=L, device=dev)
    _check(scorer.score([rows[i] for i in g["cand"]], [rows[i] for i in g["ref"]]), g, rows, "wide, ids")


def test_evaluate_bert_score_is_the_mean_of_the_pairs(dev, tiny_scorer):
    gt = {"a.mp4": {"captions": [{"sentence": "Crack the eggs into a bowl"}, {"sentence": "Whisk"}]},
          "b.mp4": {"captions": [{"sentence": "WHISK"}]},
          "c.mp4": {"captions": []},
          "d.mp4": {"captions": [{"sentence": "paint the wall"}, {"sentence": ""}]}}
    pred = {"a.mp4": {"captions": [{"sentence": "crack two eggs"}, {"sentence": "Stir the eggs"}]},
            "b.mp4": {"captions": [{"sentence": "stir the eggs"}]},
            "c.mp4": {"captions": []},
            "d.mp4": {"captions": [{"sentence": "Paint The Wall"}, {"sentence": "wait"}]}}
    cats = {"a.mp4": "Food", "b.mp4": "Food", "c.mp4": "Pets", "d.mp4": "Home"}
    cands = ["crack two eggs", "stir the eggs", "stir the eggs", "paint the wall", "wait"]
    refs = ["crack the eggs into a bowl", "whisk", "whisk", "paint the wall", ""]
    F = tiny_scorer.score(cands, refs)[2]
    assert F[3] > 0.99 and F[4] == 0 and torch.equal(F[1], F[2])
    stats = {}
    res = evaluation.evaluate_bert_score(gt, pred, cats, tiny_scorer, per_category=True, stats=stats)
    assert res == {"Food": {"BERTScore_F1": F[:3].mean().item(), "Total": 2}, "Home": {"BERTScore_F1": F[3:].mean().item(), "Total": 1},
                   "all": {"BERTScore_F1": F.mean().item(), "Total": 4}}
    assert stats["pairs"] == 5 and stats["unique_sentences"] == 7             # every unique sentence once, one launch for all pairs
    assert evaluation.evaluate_bert_score(gt, pred, cats, tiny_scorer) == {"all": res["all"]}


def test_sentence_transformer_bits_are_unchanged_by_a_scorer(dev, bpe):
    from hirest_amd.sentence_encoder import SentenceTransformer
    g = np.load(os.path.join(GOLDEN, "minilm_tiny.npz"))
    rows = [r.tolist() for r in np.split(g["ids"], np.cumsum(g["lens"])[:-1])]
    cfg = synth.MINILM_TINY
    st = SentenceTransformer(config=cfg, state_dict=synth.bert_state_dict(cfg, int(g["seed"])), device=dev)
    before = st.encode_ids(rows).clone()
    assert np.abs(before.cpu().numpy() - g["emb"]).max() < 1e-5
    t = np.load(os.path.join(GOLDEN, "bertscore_tiny.npz"))
    rc, L = synth.ROBERTA_TINY, int(t["num_layers"])
    scorer = bert_score.BERTScorer(config=rc, state_dict=synth.roberta_state_dict(rc, int(t["seed"]), L), num_layers=L,
                                   vocab=bpe["vocab"], merges=bpe["merges"], device=dev)
    scorer.score(["crack the eggs", ""], ["whisk the eggs", "stir"])
    assert torch.equal(st.encode_ids(rows), before)
