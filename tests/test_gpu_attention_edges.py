"""The bf16 attention kernels (csrc/attention.hip) at every N where the entry or a kernel takes another path — 80 | 81 (5 or 17 key tiles,
one workgroup per head or the persistent kernel), 16 k and 16 k +- 1 (the mask edge of the last key tile), 256 | 257 (the FAST switch) —
for both head widths, causal and not, through every launcher instantiation of hirest_attention_bf16_rows.

Four input families (tests/_exact_inputs.py; their preconditions are checked in tests/test_exact_inputs_host.py):
  1. selector: one key takes the whole softmax, the output row must be that key's V row bit for bit;
  2. uniform: q = 0 and an indicator V, the output is a count of visible keys over their number;
  3. isolation: the neighbouring frame and what lies after the buffer would dominate if they were ever read as keys;
  4. random, with a bound per element relative to the column's own visible maximum."""
import pytest
import torch

import _exact_inputs as X

pytestmark = pytest.mark.gpu

H = X.ATTN_H
SENT16 = 0x5A5B
GUARD_ROWS = 8
TAIL_ROWS = 32

# (B, N, dh, causal) -> variants: B = 3 takes launch (variant 1) and launch2 (2, and 7 below 64 frames); B = 64 with N > 80 takes launch3 for 3..7
GRID = [(3, N, dh, c, (1, 2, 7)) for dh in (64, 88) for c in (False, True) for N in X.ATTN_N] + \
       [(64, N, dh, c, (3, 4, 5, 6, 7)) for dh in (64, 88) for c in (False, True) for N in X.ATTN_N if N > 80]
GRID_IDS = [f"B{B}-N{N}-dh{dh}-{'causal' if c else 'full'}" for B, N, dh, c, _ in GRID]
grid = pytest.mark.parametrize("B,N,dh,causal,variants", GRID, ids=GRID_IDS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def test_grid_reaches_every_launcher_instantiation():
    """X.attention_launcher is the dispatch of hirest_attention_bf16_rows, copied: the grid above reaches every (launcher, DH, NT, FAST,
    causal) there is, and the 64-frame cases are exactly those that reach launch3."""
    reached = {X.attention_launcher(v, B, N, dh, c) for B, N, dh, c, vs in GRID for v in vs}
    assert reached == X.attention_launchers_all()
    for B, N, dh, c, vs in GRID:
        for v in vs:
            assert (X.attention_launcher(v, B, N, dh, c)[0] == "launch3") == (B == 64)


def _bits(t):
    return t.view(torch.int16)


def _sentinel(rows, cols, dev):
    return torch.full((rows, cols), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _attention(variant, qkv, out, B, N, dh, causal, q_rows=None):
    """hirest_attention_bf16_rows on raw pointers (qkv / out may be views of larger allocations) under one kernel selection."""
    from hirest_amd import _lib, ops
    ops.attention_select_kernel(variant)
    try:
        _lib.check(_lib.load().hirest_attention_bf16_rows(qkv.data_ptr(), out.data_ptr(), B, N, H, dh, dh ** -0.5, int(causal),
                                                          N if q_rows is None else q_rows, ops.stream_ptr()), "hirest_attention_bf16_rows")
    finally:
        ops.attention_select_kernel(ops.ATTENTION_DEFAULT_KERNEL)
    return out


def _run(variant, qkv_dev, B, N, dh, causal, dev):
    """One full call into a buffer with sentinel guard rows; returns the B * N output rows after checking the guard."""
    buf = _sentinel(B * N + GUARD_ROWS, H * dh, dev)
    _attention(variant, qkv_dev, buf, B, N, dh, causal)
    assert (_bits(buf[B * N:]) == SENT16).all(), "rows after the output were written"
    return buf[:B * N]


@grid
def test_selector_is_bit_exact(dev, B, N, dh, causal, variants):
    """Family 1: out[b, i, h] == v[b, pi(i), h] bit for bit — a wrong key, head, frame or row index anywhere, or a mask that hides key
    pi(i) (key N - 1 and the tile edges included), gives another row."""
    for seed in ((0, 1, 2) if B == 3 else (0,)):
        d = X.attn_selector(B, N, H, dh, causal, seed)
        qkv, want = d["qkv"].to(dev), d["want"].to(dev)
        for v in variants:
            out = _run(v, qkv, B, N, dh, causal, dev)
            assert torch.equal(_bits(out), _bits(want)), (v, seed)


@grid
def test_uniform_counts_keys(dev, B, N, dh, causal, variants):
    """Family 2: |out - count / keys| <= ulp_bf16(ref) / 2 + 2^-19 |ref| + 2^-24 per element (X.uniform_bound, where the derivation is
    written out); one key too many or too few is off by >= 19 % in its column.  Where the number of visible keys is a power of two the
    quotient is a bf16 number and the result is exact.  Worst error / bound observed on the MI355X over the grid: 0.995."""
    d = X.attn_uniform(B, N, H, dh, causal, 0)
    qkv, ref = d["qkv"].to(dev), d["ref"]
    keys = d["keys"]
    pow2 = ((keys & (keys - 1)) == 0).repeat(B)                                     # per output row
    worst = 0.0
    for v in variants:
        out = _run(v, qkv, B, N, dh, causal, dev).cpu().double()
        ratio = ((out - ref).abs() / X.uniform_bound(ref)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (v, ratio)
        assert torch.equal(out[pow2], ref[pow2]), v
    print(f"uniform B={B} N={N} dh={dh} causal={causal}: worst error / bound {worst:.4f}")


@grid
def test_isolation_from_neighbours_and_tail(dev, B, N, dh, causal, variants):
    """Family 3.  The packed activation is a view of a larger allocation whose TAIL_ROWS trailing rows hold NaN in Q and V and 3e38 in K, and
    a key of the neighbouring frame would meet a logit 400 above the real ones: the result is finite and within the per-element bound of
    family 4 against fp64, bit-identical to the same call on a buffer without the poisoned tail, and leaves the guard rows alone.
    hirest_attention_bf16_rows with q_rows in {1, 33, N} writes the same bits to rows below q_rows and leaves the rows from q_rows on alone.
    (Reads and writes of allocated memory only.)  Worst error / bound observed on the MI355X over the grid: 0.598."""
    D = H * dh
    d = X.attn_isolation(B, N, H, dh, causal, 0)
    clean = d["qkv"].to(dev)
    big = torch.empty((B * N + TAIL_ROWS, 3 * D), dtype=torch.bfloat16, device=dev)
    big[:B * N] = clean
    big[B * N:, :D] = float("nan")
    big[B * N:, D:2 * D] = 3e38
    big[B * N:, 2 * D:] = float("nan")
    poisoned = big[:B * N]
    ref = X.attention_ref(d["qkv"], B, N, H, dh, causal)
    bound = X.attention_bound(X.column_max_admitted(d["qkv"], B, N, H, dh, causal))
    worst = 0.0
    for v in variants:
        out = _run(v, poisoned, B, N, dh, causal, dev)
        assert torch.isfinite(out.float()).all(), v
        assert torch.equal(_bits(out), _bits(_run(v, clean, B, N, dh, causal, dev))), v
        ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (v, ratio)
        for q_rows in sorted({1, 33, N}):
            if q_rows > N:
                continue
            part = _sentinel(B * N + GUARD_ROWS, D, dev)
            _attention(v, poisoned, part, B, N, dh, causal, q_rows=q_rows)
            assert (_bits(part[B * N:]) == SENT16).all(), (v, q_rows)
            part = part[:B * N].reshape(B, N, D)
            assert torch.equal(_bits(part[:, :q_rows]), _bits(out.reshape(B, N, D)[:, :q_rows])), (v, q_rows)
            assert (_bits(part[:, q_rows:]) == SENT16).all(), (v, q_rows)
    print(f"isolation B={B} N={N} dh={dh} causal={causal}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("qscale", [1.0, 6.0])
@grid
def test_random_inputs_per_element(dev, B, N, dh, causal, variants, qscale):
    """Family 4: |out[b, i, h, d] - ref| <= 2 * 2^-8 * max over visible j of |v[b, j, h, d]| (X.attention_bound: three bf16 roundings of at
    most 2^-9 each relative to that column maximum — P, the fp32 normaliser's mismatch with the rounded P, the output — and 2^-9 for the
    fp32 score and exp2 error).  V columns 1 and 2 of every head are scaled by 64 and 1 / 64, so each column is held to its own scale.
    Worst error / bound observed on the MI355X over the grid and both q scales: 0.605."""
    d = X.attn_random(B, N, H, dh, causal, qscale)
    qkv = d["qkv"].to(dev)
    ref = X.attention_ref(d["qkv"], B, N, H, dh, causal)
    bound = X.attention_bound(X.column_max_admitted(d["qkv"], B, N, H, dh, causal))
    worst = 0.0
    for v in variants:
        out = _run(v, qkv, B, N, dh, causal, dev).cpu().double()
        ratio = ((out - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (v, ratio)
    print(f"random B={B} N={N} dh={dh} causal={causal} qscale={qscale}: worst error / bound {worst:.4f}")
