"""BERTScore's cosine and greedy-matching steps in numpy float64, one pair at a time over its real tokens only: the yardstick of the
fixture generator (tests/golden/make_bertscore_golden.py) and of the host and GPU tests.  No model, no device."""
import numpy as np


def pair_scores(c, r, wc, wr):
    """c [Lc, D], r [Lr, D] token states; wc [Lc], wr [Lr] token weights -> (P, R, F, min over all row and column maxima)"""
    c = np.asarray(c, np.float64)
    r = np.asarray(r, np.float64)
    c = c / np.sqrt((c * c).sum(1, keepdims=True))
    r = r / np.sqrt((r * r).sum(1, keepdims=True))
    sim = c @ r.T
    wp, wrec = sim.max(1), sim.max(0)
    wc, wr = np.asarray(wc, np.float64), np.asarray(wr, np.float64)
    P = float((wc * wp).sum() / wc.sum()) if wc.sum() != 0 else 0.0
    R = float((wr * wrec).sum() / wr.sum()) if wr.sum() != 0 else 0.0
    F = 2 * P * R / (P + R) if P + R != 0 else 0.0
    return P, R, F, float(min(wp.min(), wrec.min()))


def greedy(states, seq_off, weight, cand_seq, ref_seq):
    """The contract of hirest_bertscore_greedy in float64: [n_pairs, 3]; a sentence id outside [0, n_seq) gives NaNs."""
    n_seq = len(seq_off) - 1
    out = np.full((len(cand_seq), 3), np.nan)
    for p, (a, b) in enumerate(zip(cand_seq, ref_seq)):
        if not (0 <= a < n_seq and 0 <= b < n_seq):
            continue
        sa, sb = slice(seq_off[a], seq_off[a + 1]), slice(seq_off[b], seq_off[b + 1])
        out[p] = pair_scores(states[sa], states[sb], weight[sa], weight[sb])[:3]
    return out


def special_weights(seq_off):
    """idf=False: 1 per token, 0 for each sentence's first and last"""
    seq_off = np.asarray(seq_off, np.int64)
    w = np.ones(int(seq_off[-1]), np.float32)
    w[seq_off[:-1]] = 0
    w[seq_off[1:] - 1] = 0
    return w
