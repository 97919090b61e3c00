"""Host-side pieces of step captioning.  caption_search.beam_layout: the one statement of the packed beam-state buffers.  MomentModel._trim_index_table (the vectorised form test_step_captioning uses) against the per-sample list walk _trim_index, which restates
trim_feats (modeling.py:529-554): more selected frames than slots -> the first max_frames; fewer -> frame j repeated
(j + 1) F // N - j F // N times; none -> zero rows (-1)."""
import random

import pytest
import torch

from hirest_amd.moment_model import MomentModel


def test_trim_index_table_equals_the_list_walk():
    rng = random.Random(7)
    for trial in range(600):
        B, T, F = rng.randint(1, 6), rng.randint(1, 90), rng.choice([1, 2, 5, 20, 33])
        dens = rng.random()
        mask = torch.tensor([[1 if rng.random() < dens else 0 for _ in range(T)] for _ in range(B)], dtype=torch.long)
        if trial % 7 == 0:
            mask[0] = 0                                   # an empty moment
        if trial % 11 == 0:
            mask[-1] = 1                                  # every frame selected
        if trial % 5 == 0:
            mask[0] = 2 * (mask[0] > 0)                   # only the value 1 selects (mask == 1 in the reference)
        want = [MomentModel._trim_index(r, F) for r in mask.tolist()]
        assert MomentModel._trim_index_table(mask, F).tolist() == want, (B, T, F)


def test_trim_index_closed_form_examples():
    # 3 selected frames into 20 slots: repeats 6, 7, 7 (floor differences of j * 20 / 3)
    mask = torch.zeros(1, 10, dtype=torch.long)
    mask[0, [2, 5, 6]] = 1
    assert MomentModel._trim_index_table(mask, 20).tolist()[0] == [2] * 6 + [5] * 7 + [6] * 7
    mask[0, :] = 1
    assert MomentModel._trim_index_table(mask, 4).tolist()[0] == [0, 1, 2, 3]


def test_caption_texts_with_and_without_a_vocabulary():
    """_caption_texts: ids as decimal strings when no BERT vocabulary is attached; with one, the reference's read-out (modeling.py:614-626:
    cut at [SEP] / [PAD], join word pieces)."""
    m = MomentModel.__new__(MomentModel)                      # the method only reads tokenizer_vocab
    m.tokenizer_vocab = None
    assert m._caption_texts([[7, 102, 5], []], True) == {"prediction": ["7 102 5", ""], "token_ids": [[7, 102, 5], []]}
    m.tokenizer_vocab = ["[PAD]", "[CLS]", "[SEP]", "cut", "##ting", "board", "##s"]
    res = m._caption_texts([[3, 4, 5, 6, 2, 3], [5, 0, 3], [2]], False)
    assert res == {"prediction": ["cutting boards", "board", ""]}


@pytest.mark.parametrize("B,beams,max_words", [(1, 1, 1), (1, 7, 3), (5, 5, 48), (32, 3, 48)])
def test_beam_layout_names_disjoint_slices_that_cover_the_buffers(B, beams, max_words):
    """ibuf = tokens | backptr | n_steps | done | ids | parents and fbuf = add | scores: in that order, back to back, of the sizes the
    kernels index them with; the host read-out copies everything in front of `done` and reset() rewrites everything from `ids` on."""
    from hirest_amd.caption_search import beam_layout
    L = beam_layout(B, beams, max_words)
    nt, R = B * max_words * beams, B * beams
    for slices, length, want in ((L.ibuf, L.ibuf_len, [("tokens", nt), ("backptr", nt), ("n_steps", B), ("done", B), ("ids", R), ("parents", R)]),
                                 (L.fbuf, L.fbuf_len, [("add", R), ("scores", R)])):
        assert list(slices) == [name for name, _ in want]
        at = 0
        for name, n in want:                              # back to back from 0: pairwise disjoint, in order
            assert (slices[name].start, slices[name].stop, slices[name].step) == (at, at + n, None), name
            at += n
        assert at == length                               # ... and they cover the buffer exactly
        assert sorted(i for s in slices.values() for i in range(length)[s]) == list(range(length))
    assert (L.readout.start, L.readout.stop) == (0, L.ibuf["done"].start) and L.readout.step is None
    assert L.reset.start == L.ibuf["ids"].start and range(L.ibuf_len)[L.reset] == range(L.ibuf["ids"].start, L.ibuf_len)
