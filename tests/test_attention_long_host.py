"""hirest_attention_bf16_long on the CPU: the entry's refusals (before any launch), the guarantees of the input families of
tests/_exact_inputs.py at the lengths tests/test_gpu_attention_long.py runs them at, and the towers' routing rule."""
import os
import re

import pytest
import torch

import _attention_long_cases as L
import _exact_inputs as X

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_PTR, BADARG, SHAPE = 1 << 20, -1, -2


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_long_entry_refuses_bad_arguments_before_any_launch(lib):
    """Placeholder pointers are never dereferenced: every call below returns from the argument checks."""
    f = lib.hirest_attention_bf16_long
    assert f(None, X_PTR, 1, 577, 2, 64, 0.125, 0, None) == BADARG
    assert f(X_PTR, None, 1, 577, 2, 64, 0.125, 0, None) == BADARG
    for B in (0, -1):
        assert f(X_PTR, X_PTR, B, 577, 2, 64, 0.125, 0, None) == BADARG
    for Hh in (0, -3):
        assert f(X_PTR, X_PTR, 1, 577, Hh, 64, 0.125, 0, None) == BADARG
    assert f(X_PTR, X_PTR, 1, 577, 2, 64, 0.125, -1, None) == BADARG
    for N in (0, -5, L.LONG_MAX + 1, 1 << 20):
        assert f(X_PTR, X_PTR, 3, N, 2, 64, 0.125, 0, None) == SHAPE
    for dh in (88, 80, 32, 128, 0):
        assert f(X_PTR, X_PTR, 3, 577, 2, dh, 0.1, 0, None) == SHAPE
        assert f(X_PTR, X_PTR, 3, 577, 2, dh, 0.1, 1, None) == SHAPE


def test_short_entries_still_refuse_long_sequences(lib):
    """The new entry does not widen the old ones: N > 272 stays HIREST_E_SHAPE there for both head widths."""
    for N in (273, 577, L.LONG_MAX):
        for dh, scale in ((64, 0.125), (88, 0.1)):
            assert lib.hirest_attention_bf16(X_PTR, X_PTR, 3, N, 2, dh, scale, 0, None) == SHAPE
            assert lib.hirest_attention_bf16_rows(X_PTR, X_PTR, 64, N, 2, dh, scale, 0, 1, None) == SHAPE


@pytest.mark.parametrize("B,N,seed", L.SELECTOR_CASES)
def test_selector_gap_at_the_long_lengths(B, N, seed):
    """The selected logit exceeds every other by more than 64, so a rescale factor between key tiles is below exp(-64) < 2^-92: whatever
    a streaming kernel accumulated before it met the selected key vanishes against that key's row in fp32."""
    d = X.attn_selector(B, N, L.H, L.DH, False, seed)
    assert X.selector_gap(d, B, N, L.H, L.DH, False) > 64
    # the wanted rows are V rows of the same frame and head, and distinct keys give distinct rows
    _, _, v = X.unpack_qkv(d["qkv"], B, N, L.H, L.DH)
    want = d["want"].reshape(B, N, L.H, L.DH)
    for b in range(B):
        for h in range(L.H):
            assert torch.equal(want[b, :, h].view(torch.int16), v[b, d["pi"][b, h], h].view(torch.int16))
            assert len({bytes(r.view(torch.int16).numpy().tobytes()) for r in v[b, :, h]}) == N


@pytest.mark.parametrize("N", L.LENGTHS)
def test_uniform_reference_at_the_long_lengths(N):
    B = 3
    d = X.attn_uniform(B, N, L.H, L.DH, False, 0)
    q, _, v = X.unpack_qkv(d["qkv"].float(), B, N, L.H, L.DH)
    assert q.abs().max().item() == 0 and set(v.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(d["keys"], torch.full((N,), N))
    ref = d["ref"].reshape(B, N, L.H, L.DH)[0, 0, 0]
    cnt = ref * N
    assert (cnt - cnt.round()).abs().max().item() < 1e-9 and cnt.min().item() >= N // L.DH
    # one key too many (the clamped duplicate of row N - 1 left unmasked) or one too few (row N - 1 dropped) in that key's column
    col = (N - 1) % L.DH
    have = ref[col]
    for wrong in ((have * N + 1) / (N + 1), (have * N - 1) / (N - 1)):
        assert abs(wrong - have) > 4 * X.uniform_bound(have).item()


@pytest.mark.parametrize("N", L.LENGTHS)
def test_isolation_logits_at_the_long_lengths(N):
    B = 3
    d = X.attn_isolation(B, N, L.H, L.DH, False, 0)
    s = X.attention_logits(d["qkv"], B, N, L.H, L.DH)
    assert s.max().item() < -150 and s.min().item() > -250
    q, k, _ = X.unpack_qkv(d["qkv"].double(), B, N, L.H, L.DH)
    for qq, kk in ((q[:-1], k[1:]), (q[1:], k[:-1])):
        # the rows a kernel would borrow first: the leading keys of the next frame, the trailing keys of the previous one
        cross = torch.einsum("bihd,bjhd->bhij", qq, torch.cat([kk[:, :64], kk[:, -64:]], 1)) * L.DH ** -0.5
        assert cross.min().item() > 150


def test_random_family_columns_keep_their_own_scale():
    B, N = 3, 577
    d = X.attn_random(B, N, L.H, L.DH, False, 6.0)
    cm = X.column_max_admitted(d["qkv"], B, N, L.H, L.DH, False).reshape(B, N, L.H, L.DH)
    assert cm[:, :, :, 1].min().item() > 64 and cm[:, :, :, 2].max().item() < 0.1


def test_tower_routing_rule():
    """The long entry is taken only for T > 272 and 64-wide heads: everything the short kernels ran before still runs on them, and what
    is routed to the new entry is exactly what it accepts."""
    for T in (1, 50, 77, 257, 272, 273, 577, 1025, L.LONG_MAX):
        for dh in (64, 88):
            assert L.tower_takes_long_entry(T, dh) == (T >= 273 and dh == 64)
    assert not L.tower_takes_long_entry(577, 88) and not L.tower_takes_long_entry(272, 64)
    src = open(os.path.join(REPO, "hirest_amd", "csrc", "tower.hip")).read()
    rule = re.search(r"inline bool vision_attention_long\(int T, int dh\) \{ return ([^;]+); \}", src)
    assert rule and rule.group(1) == "T > 272 && dh == 64"
    # the three vision call sites go through the rule; the only direct call of a short entry left outside it is the causal (text) one
    assert src.count("vision_attention(big, h, B, T, heads, dh,") == 3
    body = src.replace(src[src.index("int vision_attention("):src.index("// one pre-LN block")], "")
    assert re.findall(r"hirest_attention_bf16\w*\(big[^;]*;", body) == \
        ["hirest_attention_bf16(big, h, B, T, heads, dh, 1.0f / sqrtf((float)dh), 1, stream));"]


def test_long_sequences_lower_the_frames_per_call():
    """2048 frames of 577 tokens would be 1.18 M rows with up to 4 D columns: the towers keep a call's rows at what 2048 frames of 257
    tokens have (the size the suite runs), so no region of the workspace outgrows the indexing the short sequences already use."""
    from hirest_amd.eva_clip import _Tower
    assert _Tower._frames_limit(2048, 257) == 2048 and _Tower._frames_limit(2048, 50) == 2048 and _Tower._frames_limit(1024, 272) == 1024
    assert _Tower._frames_limit(2048, 577) == 2048 * 257 // 577 == 912
    assert _Tower._frames_limit(1024, 577) == 912 and _Tower._frames_limit(256, 577) == 256
    assert _Tower._frames_limit(2048, L.LONG_MAX + 1) >= 64
    for T in (273, 577, 1025, L.LONG_MAX + 1):
        assert _Tower._frames_limit(2048, T) * T <= max(2048 * 257, 64 * T)
