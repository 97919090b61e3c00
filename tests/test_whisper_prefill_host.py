"""The ragged multi-window prefill without a GPU: every argument error of hirest_whisper_prefill_rows and of the ragged
kernels' own entry points is HIREST_E_BADARG before any launch, the workspace grows with each of its arguments, the packing plan
(prompts, groups, windows -> hirest_whisper_prefill_seq tables, split at 4096 packed rows) is a pure function, and a cache whose
windows' rows are not contiguous is refused."""
import ctypes as C
import re
import os
import types

import pytest
import torch

from hirest_amd import _lib, synth, whisper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, SHAPE = -1, -2
X = 1 << 20                # a pointer that is never dereferenced: every call below is rejected before anything is enqueued
ENTRIES = ("hirest_embedding_varlen_fwd_f32", "hirest_attention_f32_varlen_causal", "hirest_attention_f32_varlen_cross",
           "hirest_whisper_prefill_scatter", "hirest_whisper_prefill_workspace_bytes", "hirest_whisper_prefill_rows")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def table(*seqs):
    """(offset, length, window, first_row, n_rows, sot_index) ... -> the C array"""
    return whisper._seq_table(list(seqs))


def descriptor(layers=2, heads=2, inter=512, vocab_padded=200, max_pos=48):
    """a decoder descriptor whose pointers are set and never followed; -> (descriptor, what keeps its layer array alive)"""
    L = (_lib.WhisperLayer * layers)()
    d = _lib.WhisperDecoder()
    d.layers, d.heads, d.hidden, d.inter, d.vocab_padded, d.max_pos = layers, heads, 64 * heads, inter, vocab_padded, max_pos
    d.tok_emb = d.pos_emb = d.ln_g = d.ln_b = d.lm_b = X
    d.layer = L
    return d, L


GOOD = [(0, 4, 0, 0, 1, -1), (4, 1, 1, 1, 5, -1), (5, 9, 1, 7, 3, 2)]       # 14 packed rows, 2 windows, cache rows 0, 1-5, 7-9 of 10

# one broken field at a time -> why it is refused
BROKEN = {
    "a length of zero": [(0, 0, 0, 0, 1, -1)],
    "a negative length": [(0, -3, 0, 0, 1, -1)],
    "a first sequence that does not start at row 0": [(1, 4, 0, 0, 1, -1)],
    "overlapping packed ranges": [(0, 4, 0, 0, 1, -1), (3, 2, 0, 1, 1, -1)],
    "a gap between packed ranges": [(0, 4, 0, 0, 1, -1), (5, 2, 0, 1, 1, -1)],
    "packed ranges out of order": [(4, 1, 0, 0, 1, -1), (0, 4, 0, 1, 1, -1)],
    "a sot_index past the sequence": [(0, 4, 0, 0, 1, 4)],
    "a sot_index that is the last position": [(0, 4, 0, 0, 1, 3)],
}
BROKEN_WINDOW = {"a negative window": [(0, 4, -1, 0, 1, -1)], "a window past the last": [(0, 4, 2, 0, 1, -1)]}
BROKEN_ROWS = {
    "a negative first row": [(0, 4, 0, -1, 1, -1)],
    "no cache row": [(0, 4, 0, 0, 0, -1)],
    "a row range past R": [(0, 4, 0, 8, 3, -1)],
    "row ranges that overlap": [(0, 4, 0, 2, 3, -1), (4, 1, 0, 4, 2, -1)],
    "row ranges that overlap, the later one first": [(0, 4, 0, 4, 2, -1), (4, 1, 0, 2, 3, -1)],
}


def test_entries_declared_bound_and_exported(lib):
    text = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hirest_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    fields = re.search(r"typedef struct hirest_whisper_prefill_seq \{(.*?)\} hirest_whisper_prefill_seq;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[2\])?[,;]", fields) == ["offset", "length", "window", "first_row", "n_rows", "sot_index", "reserved"]
    assert C.sizeof(_lib.WhisperPrefillSeq) == 32
    t = table(*GOOD)
    assert [(s.offset, s.length, s.window, s.first_row, s.n_rows, s.sot_index) for s in t] == GOOD


def test_prefill_rows_argument_errors_without_gpu(lib):
    d, keep = descriptor()
    P = C.c_void_p * 2
    ptrs = P(X, X)
    big = 1 << 40

    def call(seqs=GOOD, desc=d, n_seq=None, ids=X, k=ptrs, v=ptrs, R=10, T_max=12, x=ptrs, n_windows=2, Tk=33, last=X, sot=X, ws=X, ws_bytes=big):
        t = table(*seqs) if seqs is not None else None
        return lib.hirest_whisper_prefill_rows(C.byref(desc) if desc is not None else None, len(seqs) if n_seq is None else n_seq, t, ids, k, v, R,
                                               T_max, x, n_windows, Tk, last, sot, ws, ws_bytes, None)
    # a NULL pointer
    for kw in (dict(desc=None), dict(seqs=None, n_seq=3), dict(ids=None), dict(k=None), dict(v=None), dict(x=None), dict(last=None), dict(ws=None)):
        assert call(**kw) == BAD, kw
    assert call(sot=None) == BAD                                     # a sequence asks for its sot row and there is nowhere to put it
    assert call(k=P(X, None)) == BAD and call(v=P(None, X)) == BAD and call(x=P(X, None)) == BAD
    for field in ("tok_emb", "pos_emb", "ln_g", "ln_b", "lm_b"):
        broken, keep2 = descriptor()
        setattr(broken, field, None)
        assert call(desc=broken) == BAD, field
    no_layers, _ = descriptor()
    no_layers.layer = None
    assert call(desc=no_layers) == BAD
    # counts
    assert call(n_seq=0) == BAD and call(n_seq=-1) == BAD
    assert call(R=0) == BAD and call(T_max=0) == BAD and call(Tk=0) == BAD and call(n_windows=0) == BAD
    # the sequence table
    for why, seqs in {**BROKEN, **BROKEN_WINDOW, **BROKEN_ROWS}.items():
        assert call(seqs=seqs) == BAD, why
    # a length outside [1, min(max_pos, T_max)]: T_max 12 and max_pos 48 admit 12, not 13; max_pos 8 admits 8, not 9
    assert call(seqs=[(0, 13, 0, 0, 1, -1)]) == BAD
    short, keep3 = descriptor(max_pos=8)
    assert call(seqs=[(0, 9, 0, 0, 1, -1)], desc=short) == BAD
    # a workspace that is too small, by one byte
    need = lib.hirest_whisper_prefill_workspace_bytes(C.byref(d), 14, 3)
    assert need > 0 and call(ws_bytes=need - 1) == BAD and call(ws_bytes=0) == BAD
    assert call(seqs=[(0, 12, 0, 0, 1, -1)], ws_bytes=lib.hirest_whisper_prefill_workspace_bytes(C.byref(d), 12, 1) - 1) == BAD
    # a table that passes every check above is stopped by the next one: a descriptor whose width is not heads * 64
    odd, keep4 = descriptor()
    odd.hidden = 120
    assert call(desc=odd) == SHAPE


def test_ragged_kernel_entries_argument_errors_without_gpu(lib):
    emb = lambda seqs=GOOD, ids=X, tab=X, pos=X, out=X, vocab=200, max_pos=48, D=128, n_seq=None: lib.hirest_embedding_varlen_fwd_f32(
        ids, tab, pos, out, vocab, max_pos, D, table(*seqs) if seqs is not None else None, len(seqs or []) if n_seq is None else n_seq, None)
    causal = lambda seqs=GOOD, q=X, k=X, v=X, out=X, H=2, n_seq=None: lib.hirest_attention_f32_varlen_causal(
        q, 384, k, v, 384, out, table(*seqs) if seqs is not None else None, len(seqs or []) if n_seq is None else n_seq, H, 0.125, 0.0, -1e30, None)
    cross = lambda seqs=GOOD, q=X, kv=X, out=X, H=2, n_windows=2, Tk=33, n_seq=None: lib.hirest_attention_f32_varlen_cross(
        q, 128, kv, 256, 33 * 256, n_windows, Tk, out, table(*seqs) if seqs is not None else None, len(seqs or []) if n_seq is None else n_seq, H,
        0.125, 0.0, None)
    scatter = lambda seqs=GOOD, k=X, v=X, kc=X, vc=X, R=10, T_max=12, D=128, n_seq=None: lib.hirest_whisper_prefill_scatter(
        k, v, 384, kc, vc, R, T_max, D, table(*seqs) if seqs is not None else None, len(seqs or []) if n_seq is None else n_seq, None)
    for fn, pointers in ((emb, ("ids", "tab", "pos", "out")), (causal, ("q", "k", "v", "out")), (cross, ("q", "kv", "out")),
                         (scatter, ("k", "v", "kc", "vc"))):
        for name in pointers:
            assert fn(**{name: None}) == BAD, name
        assert fn(seqs=None, n_seq=3) == BAD and fn(n_seq=0) == BAD and fn(n_seq=-2) == BAD
        for why, seqs in BROKEN.items():
            assert fn(seqs=seqs) == BAD, why
    for why, seqs in BROKEN_WINDOW.items():
        assert cross(seqs=seqs) == BAD, why
    for why, seqs in BROKEN_ROWS.items():
        assert scatter(seqs=seqs) == BAD, why
    assert emb(vocab=0) == BAD and emb(max_pos=0) == BAD and emb(D=0) == BAD and emb(D=126) == BAD and emb(max_pos=8) == BAD      # 9 > 8 positions
    assert causal(H=0) == BAD and cross(H=0) == BAD and cross(Tk=0) == BAD and cross(n_windows=0) == BAD
    assert scatter(R=0) == BAD and scatter(T_max=0) == BAD and scatter(T_max=8) == BAD and scatter(D=0) == BAD and scatter(D=130) == BAD


def test_workspace_grows_with_each_argument(lib):
    d, keep = descriptor()
    ws = lambda desc=d, N=100, n_seq=3: lib.hirest_whisper_prefill_workspace_bytes(C.byref(desc) if desc is not None else None, N, n_seq)
    al = lambda v: (v + 255) // 256 * 256
    # seven activations of N rows (x, a, b, ln, ctx: D; q | k | v: 3 D; the MLP's: inter), the gathered rows of the head, no split-form scratch
    assert ws() == 5 * al(100 * 128 * 4) + al(100 * 384 * 4) + al(100 * 512 * 4) + al(2 * 3 * 128 * 4)
    assert ws(N=101) > ws() and ws(n_seq=4) > ws() and ws(N=4096) > ws(N=4095)
    wide, k2 = descriptor(heads=4)
    deep, k3 = descriptor(inter=1024)
    assert ws(desc=wide) > ws() and ws(desc=deep) > ws()
    assert ws(desc=None) == 0 and ws(N=0) == 0 and ws(n_seq=0) == 0
    # where a layer's product takes the split form of hirest_gemm_f32_ws (few 64 x 64 tiles, K >= 1024), its scratch is part of the plan
    small_en, k4 = descriptor(heads=12, inter=3072, vocab_padded=51864, max_pos=448)
    split = lib.hirest_gemm_f32_workspace_bytes(300, 768, 3072)
    assert split == 4 * 300 * 768 * 4
    assert ws(desc=small_en, N=300, n_seq=2) == 5 * al(300 * 768 * 4) + al(300 * 2304 * 4) + al(300 * 3072 * 4) + al(2 * 2 * 768 * 4) + al(split)


def test_packing_plan():
    plan = whisper.prefill_plan
    # a prompt of one token
    assert plan([[7]], [0], [1], [0]) == [[(0, 1, 0, 0, 1, -1)]]
    # two sequences on one window, the groups' rows one after the other; a sot index that is the last position is not asked for twice
    prompts = [[1, 2, 3, 4], [5], list(range(9))]
    assert plan(prompts, [0, 1, 7], [1, 5, 3], [0, 1, 1], [3, None, 2]) == [GOOD]
    assert plan(prompts, [0, 1, 7], [1, 5, 3], [0, 1, 1]) == [[s[:5] + (-1,) for s in GOOD]]
    # the 4096-row split falls between sequences and offsets restart: 9 prompts of 448 tokens fit a call, the tenth opens the next
    long = [[0] * 448] * 11
    calls = plan(long, list(range(11)), [1] * 11, list(range(11)))
    assert [len(c) for c in calls] == [9, 2] and whisper.PREFILL_ROWS_PER_CALL == 4096
    assert [s[0] for s in calls[0]] == [448 * i for i in range(9)] and [s[0] for s in calls[1]] == [0, 448]
    assert [s[2] for s in calls[1]] == [9, 10] and [s[3] for s in calls[1]] == [9, 10]
    assert sum(s[1] for s in calls[0]) <= 4096 < sum(s[1] for s in calls[0]) + 448
    # a sequence that would cross the limit moves whole; one that alone exceeds it still gets a call of its own
    assert [[s[1] for s in c] for c in plan([[0] * 5, [0] * 4, [0] * 3], [0, 1, 2], [1, 1, 1], [0, 0, 0], rows_per_call=8)] == [[5], [4, 3]]
    assert [[s[1] for s in c] for c in plan([[0] * 9, [0] * 2], [0, 1], [1, 1], [0, 0], rows_per_call=8)] == [[9], [2]]
    for bad in (dict(prompts=[]), dict(prompts=[[]]), dict(first_rows=[0, 1]), dict(sot=[1]), dict(sot=[-1])):
        with pytest.raises(ValueError):
            plan(bad.get("prompts", [[1]]), bad.get("first_rows", [0]), [1], [0], bad.get("sot"))
    # every table of a plan passes the C side's checks up to the first launch (a NULL decoder is what then stops the call)
    lib = _lib.load()
    for c in calls:
        t = whisper._seq_table(c)
        assert lib.hirest_whisper_prefill_scatter(X, X, 384, X, X, 11, 448, 0, t, len(c), None) == BAD       # D = 0, checked first
        assert lib.hirest_whisper_prefill_scatter(X, X, 382, X, X, 11, 448, 128, t, len(c), None) == SHAPE    # the table passed; the stride did not


def test_window_rows_must_be_contiguous():
    rr = whisper.window_row_ranges
    assert rr([0, 0, 0, 1, 1], 2) == [(0, 3), (3, 2)] and rr([1, 0, 0], 2) == [(1, 2), (0, 1)] and rr([0], 1) == [(0, 1)]
    for rows, n in (([0, 1, 0], 2), ([0, 0, 1, 1, 0], 2), ([0, 0], 2), ([0, 2], 2), ([0, -1], 2)):
        with pytest.raises(ValueError):
            rr(rows, n)
    # prefill() refuses such a cache before it touches the device
    cfg, eot, seed, _ = synth.WHISPER_DEC_CASES["p"]
    dec = whisper.TextDecoder(cfg, synth.whisper_decoder_state_dict(cfg, seed))
    kc = types.SimpleNamespace(length=0, n_windows=2, T_max=8, R=3, row_window=torch.tensor([0, 1, 0]))
    with pytest.raises(ValueError, match="not contiguous"):
        dec.prefill(torch.zeros((2, 4), dtype=torch.int32), kc)
    with pytest.raises(ValueError, match="one prompt per window"):
        dec.prefill(torch.zeros((3, 4), dtype=torch.int32), types.SimpleNamespace(length=0, n_windows=2, T_max=8, R=3, row_window=torch.tensor([0, 0, 1])))
    with pytest.raises(ValueError, match="does not fit"):
        dec.prefill_many([[1] * 9], types.SimpleNamespace(T_max=8), [0], [1], [0])
