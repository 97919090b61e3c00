"""hirest_attention_bf16_long (csrc/attention_long.hip), the streaming bf16 attention for sequences past the short kernels' 272 tokens, on the
four input families of tests/_exact_inputs.py (their guarantees at these lengths: tests/test_attention_long_host.py):
  1. selector: one key takes the whole softmax; the output row is that key's V row bit for bit, whatever tile the key sits in;
  2. uniform: q = 0 and an indicator V; the output counts the visible keys, one too many or too few is a 20 % error;
  3. isolation: a key of the neighbouring frame, or of the rows after the buffer, would take the whole softmax;
  4. random, with a bound per element relative to the column's own maximum.
Lengths: 273 (first the short entries refuse), 320 (whole 64-key tiles), 321 (one key past), 577 (ViT-L/14@336px), 1025 (many tiles + 1)."""
import pytest
import torch

import _attention_long_cases as L
import _exact_inputs as X

pytestmark = pytest.mark.gpu

H, DH = L.H, L.DH
D = H * DH
SENT16 = 0x5A5B
GUARD_ROWS = 8
TAIL_ROWS = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16)


def _sentinel(rows, dev):
    return torch.full((rows, D), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _call(qkv, out, B, N, q_rows=0):
    from hirest_amd import _lib, ops
    _lib.check(_lib.load().hirest_attention_bf16_long(qkv.data_ptr(), out.data_ptr(), B, N, H, DH, DH ** -0.5, q_rows, ops.stream_ptr()),
               "hirest_attention_bf16_long")


def _run(qkv_dev, B, N, dev, q_rows=0):
    """One call into a sentinel-filled buffer with guard rows after it; returns the [B * N, D] rows after checking the guard."""
    buf = _sentinel(B * N + GUARD_ROWS, dev)
    _call(qkv_dev, buf, B, N, q_rows)
    assert (_bits(buf[B * N:]) == SENT16).all(), "rows after the output were written"
    return buf[:B * N]


@pytest.mark.parametrize("B,N,seed", L.SELECTOR_CASES)
def test_selector_is_bit_exact(dev, B, N, seed):
    """Family 1: out[b, i, h] == v[b, pi(i), h] bit for bit.  The selected logit is more than 64 above every other, so a rescale factor
    is below exp(-64) < 2^-92: the partial sums of the tiles before the selected key vanish against it in fp32, p of that key is exactly 1
    and so is the normaliser.  With q_rows in {1, 17} the rows below q_rows carry the same bits and everything else keeps the sentinel."""
    d = X.attn_selector(B, N, H, DH, False, seed)
    qkv, want = d["qkv"].to(dev), d["want"].to(dev)
    out = _run(qkv, B, N, dev)
    assert torch.equal(_bits(out), _bits(want))
    for q_rows in L.Q_ROWS:
        part = _run(qkv, B, N, dev, q_rows).reshape(B, N, D)
        assert torch.equal(_bits(part[:, :q_rows]), _bits(want.reshape(B, N, D)[:, :q_rows])), q_rows
        assert (_bits(part[:, q_rows:]) == SENT16).all(), q_rows


@pytest.mark.parametrize("B", L.BATCHES)
@pytest.mark.parametrize("N", L.LENGTHS)
def test_uniform_counts_keys(dev, B, N):
    """Family 2: |out - count / N| <= X.uniform_bound.  Every p is exactly 1 and every rescale factor exactly 1, so the accumulators hold
    integers: a masked key that counted, or a real key of the ragged last tile that did not, moves its column by about 20 %."""
    d = X.attn_uniform(B, N, H, DH, False, 0)
    out = _run(d["qkv"].to(dev), B, N, dev).cpu().double()
    ratio = ((out - d["ref"]).abs() / X.uniform_bound(d["ref"])).max().item()
    print(f"long uniform B={B} N={N}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("N", L.LENGTHS)
def test_isolation_from_neighbours_and_tail(dev, N):
    """Family 3, B = 3.  The activation is a view of a larger allocation whose trailing rows hold NaN in Q and V and 3e38 in K, and a key
    of a neighbouring frame would meet a logit 400 above the real ones.  The result is finite, within X.attention_bound of fp64, equal bit
    for bit to the call on a buffer without the poisoned tail and to a second run; frame 1 equals the same frame run alone."""
    B = 3
    d = X.attn_isolation(B, N, H, DH, False, 0)
    clean = d["qkv"].to(dev)
    big = torch.empty((B * N + TAIL_ROWS, 3 * D), dtype=torch.bfloat16, device=dev)
    big[:B * N] = clean
    big[B * N:, :D] = float("nan")
    big[B * N:, D:2 * D] = 3e38
    big[B * N:, 2 * D:] = float("nan")
    out = _run(big[:B * N], B, N, dev)
    assert torch.isfinite(out.float()).all()
    ref = X.attention_ref(d["qkv"], B, N, H, DH, False)
    bound = X.attention_bound(X.column_max_admitted(d["qkv"], B, N, H, DH, False))
    ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
    print(f"long isolation N={N}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(out, _run(clean, B, N, dev))
    assert torch.equal(out, _run(big[:B * N], B, N, dev))
    alone = _run(clean[N:2 * N].clone(), 1, N, dev)
    assert torch.equal(out[N:2 * N], alone)
    last = _run(big[2 * N:3 * N], 1, N, dev)                           # the last frame alone, the poisoned rows right behind it
    assert torch.equal(out[2 * N:], last)


@pytest.mark.parametrize("qscale", [1.0, 6.0])
@pytest.mark.parametrize("B", L.BATCHES)
@pytest.mark.parametrize("N", L.LENGTHS)
def test_random_inputs_per_element(dev, B, N, qscale):
    """Family 4: |out - ref| <= X.attention_bound(column maximum) per element, the bound the short kernels are held to (three bf16
    roundings; the running rescale works in fp32 and adds nothing a bf16 rounding would see).  The short kernels measure 0.605 of it; worst
    error / bound observed for this kernel on the MI355X: 0.410 (q scale 6), 0.100 (q scale 1); isolation inputs 0.087."""
    d = X.attn_random(B, N, H, DH, False, qscale)
    ref = X.attention_ref(d["qkv"], B, N, H, DH, False)
    bound = X.attention_bound(X.column_max_admitted(d["qkv"], B, N, H, DH, False))
    out = _run(d["qkv"].to(dev), B, N, dev)
    ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
    print(f"long random B={B} N={N} qscale={qscale}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0
    # rows of a q_rows call are the rows of the full call
    part = _run(d["qkv"].to(dev), B, N, dev, 17).reshape(B, N, D)
    assert torch.equal(part[:, :17], out.reshape(B, N, D)[:, :17]) and (_bits(part[:, 17:]) == SENT16).all()


def test_upper_edge_and_short_lengths(dev):
    """The entry's own range: N = 4096 (64 key tiles, 32 query tiles) and lengths the towers never route here (1, 64, 65) against fp64."""
    for B, N in ((1, 4096), (2, 1), (2, 64), (2, 65)):
        d = X.attn_random(B, N, H, DH, False, 1.0)
        ref = X.attention_ref(d["qkv"], B, N, H, DH, False)
        bound = X.attention_bound(X.column_max_admitted(d["qkv"], B, N, H, DH, False))
        out = _run(d["qkv"].to(dev), B, N, dev)
        ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
        print(f"long random B={B} N={N}: worst error / bound {ratio:.4f}")
        assert ratio <= 1.0
