"""The preconditions of tests/_exact_inputs.py, checked on the CPU: the GPU tests that use these generators (test_gpu_gemm_exact.py,
test_gpu_attention_edges.py, test_gpu_attention_x3_exact.py, test_gpu_gemm_f32_exact.py) assert bit equality or derived bounds that only mean
something while these hold."""
import ctypes
import math

import pytest
import torch

import _exact_inputs as X


@pytest.mark.parametrize("M,N,K", X.GEMM_SHAPES)
def test_gemm_integer_inputs_are_exact_in_fp32(M, N, K):
    d = X.gemm_exact(M, N, K)
    a, w = d["a"].float(), d["w"].float()
    assert a.abs().max() <= 3 and w.abs().max() <= 3 and torch.equal(a, a.round()) and torch.equal(w, w.round())
    for t in (d["bias"], d["resid"], d["pos"]):
        assert t.abs().max() <= 8 and torch.equal(t, t.round())
    # every partial sum is an integer of magnitude <= 9 K (+ 16 for bias and residual): far below 2^24, so fp32 holds it in any order
    assert 9 * K + 16 < X.F32_EXACT and K <= 6144
    ref64 = a.double() @ w.double().t()
    assert torch.equal(d["ref"].double(), ref64)                        # fp32 matmul == fp64 matmul
    assert ref64.abs().max().item() + 16 < X.F32_EXACT
    assert d["pos"].shape == (d["P"] + 1, N) and M % d["P"] == 0
    # the bf16 epilogue must round to nearest even: the data holds exact ties (halfway between two bf16 numbers) whose two neighbours
    # differ, so round-half-away and truncation both give other bits somewhere
    t = d["ref"] + d["bias"]
    ties = X.bf16_ties(t)
    assert ties.any(), "no exact bf16 tie in a w^T + bias"
    rne = t.to(torch.bfloat16).float()
    trunc = (t.view(torch.int32) & ~0xFFFF).view(torch.float32)
    away = torch.where(ties, trunc + (t - trunc) * 2, rne)
    assert (ties & (rne != trunc)).any() and (ties & (rne != away)).any()      # ties that round up, and ties that round down
    assert (ref64 + d["resid"].double() + d["bias"].double()).abs().max().item() < X.F32_EXACT


@pytest.mark.parametrize("M,N,K", X.GEMM_LNSTATS_SHAPES)
def test_lnstats_row_sums_are_exact(M, N, K):
    """Sums of x and x^2 over a row of the bf16-rounded stream stay integers below 2^24, and the stream holds bf16 ties."""
    d = X.gemm_lnstats(M, N, K)
    assert M >= 64 and N >= 256 and N % 8 == 0
    ref64 = d["a"].double() @ d["w"].double().t()
    assert torch.equal(d["ref"].double(), ref64)
    x = d["ref"] + d["bias"] + d["resid"]
    assert torch.equal(x.double(), ref64 + d["bias"].double() + d["resid"].double())
    assert X.bf16_ties(x).any()
    xb = x.to(torch.bfloat16).double()
    assert torch.equal(xb, xb.round())
    assert (xb * xb).sum(1).max().item() < X.F32_EXACT and xb.abs().sum(1).max().item() < X.F32_EXACT
    var = (xb * xb).mean(1) - xb.mean(1) ** 2
    assert (var / (xb * xb).mean(1)).min().item() >= 2.0 ** -20        # (no cancellation in E x^2 - mean^2 worth speaking of)


@pytest.mark.parametrize("M,N,K", X.GEMM_GELU_SHAPES + [X.X3_GELU_SHAPE])
def test_gelu_pre_activation_is_exact_and_spread(M, N, K):
    d = X.gemm_gelu(M, N, K)
    a, w = d["a"].float(), d["w"].float()
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set((w * 2.0 ** d["s"]).unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert torch.equal(d["bias"] * 8, (d["bias"] * 8).round())
    x64 = a.double() @ w.double().t() + d["bias"].double()
    assert torch.equal(d["x"].double(), x64)
    # multiples of 2^-s (s <= 3 with the bias) of magnitude <= K + 2: exact in fp32 in any order
    assert d["s"] <= 3 and (K + 2) * 8 < X.F32_EXACT
    assert 2.0 <= x64.std().item() <= 4.5
    ax = x64.abs()
    assert ((ax >= 0.25) & (ax <= 6)).double().mean().item() >= 0.25
    assert (x64 < -6).any() and (x64 > 6).any()


def test_gelu_bound_terms():
    g = torch.tensor([0.0, 1.0, 1.5, 2.0, -0.17, 255.0, 1e-9], dtype=torch.float64)
    assert X.ulp_bf16(g).tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -10, 1.0, 2.0 ** -37]
    for v in (1.0, 1.5, -0.17, 255.0):
        b = torch.tensor([v], dtype=torch.bfloat16)
        nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
        assert abs(nxt.item() - b.item()) == X.ulp_bf16(b.double()).item()
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    assert (X.gelu_ref(x) - torch.nn.functional.gelu(x)).abs().max().item() < 1e-15


@pytest.mark.parametrize("M,N,K", X.X3_SHAPES)
@pytest.mark.parametrize("frac_in_a", [True, False])
def test_x3_inputs_split_exactly(M, N, K, frac_in_a):
    d = X.gemm_x3(M, N, K, frac_in_a)
    for name in ("a", "w"):
        x, x2 = d[name], d[name + "2"]
        assert x2.shape == (x.shape[0], 2 * K) and x2.dtype == torch.bfloat16
        assert torch.equal(X.unsplit2_cpu(x2), x)                        # hi + lo is the fp32 value, exactly
        blocks = x2.reshape(x.shape[0], K // 32, 2, 32)
        assert torch.equal(blocks[:, :, 0].reshape(x.shape), x.to(torch.bfloat16))
    frac, whole = ("a", "w") if frac_in_a else ("w", "a")
    lo = lambda t: t.reshape(t.shape[0], K // 32, 2, 32)[:, :, 1]
    assert lo(d[whole + "2"]).float().abs().max().item() == 0            # one operand has lo == 0: the dropped lo * lo term is 0
    assert lo(d[frac + "2"]).float().abs().max().item() > 0              # ... and the other one exercises the hi * lo path
    # everything is a multiple of 2^-10; |sum| * 2^10 < 2^24 keeps every partial sum an fp32 number
    bound = (d["a"].double().abs() @ d["w"].double().abs().t()).max().item() + 16
    assert bound * 2 ** 10 < X.F32_EXACT
    assert torch.equal(d["ref"].double(), d["a"].double() @ d["w"].double().t())
    assert torch.equal(d["ref"] * 2 ** 10, (d["ref"] * 2 ** 10).round())


@pytest.mark.parametrize("dh", [64, 88])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N", X.ATTN_N)
def test_selector_gap(N, dh, causal):
    B, H = 3, X.ATTN_H
    d = X.attn_selector(B, N, H, dh, causal, 0)
    assert X.selector_gap(d, B, N, H, dh, causal) >= 64
    pi = d["pi"]
    if causal:
        assert (pi <= torch.arange(N)).all() and (pi[:, :, 0::3] == torch.arange(N)[0::3]).all() and (pi[:, :, 1::3] == 0).all()
    else:
        assert torch.equal(pi.sort(-1).values, torch.arange(N).expand(B, H, N))
    _, _, v = X.unpack_qkv(d["qkv"], B, N, H, dh)
    assert (v.float() != 0).all()
    rows = v.permute(0, 2, 1, 3).reshape(B * H * N, dh).view(torch.int16)
    assert torch.unique(rows, dim=0).shape[0] == B * H * N               # no two (frame, head, key) rows of v agree
    # the fp64 reference agrees: softmax puts everything on pi(i)
    ref = X.attention_ref(d["qkv"], B, N, H, dh, causal)
    assert torch.equal(ref.to(torch.bfloat16).view(torch.int16), d["want"].view(torch.int16))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_selector_keys_are_nearly_orthogonal(seed):
    """+-1 keys at N = 272, dh = 64, 3 frames: max off-diagonal |k_i . k_j| <= 40, i.e. every other logit <= 32 * 40 / 8 = 160 = 256 - 96.
    The 64-frame cases have 20 times as many pairs and reach 44 or so; what they need is the gap of 64 (|k_i . k_j| <= 48)."""
    N, H, dh = 272, X.ATTN_H, 64
    d = X.attn_selector(3, N, H, dh, False, seed)
    _, k, _ = X.unpack_qkv(d["qkv"].float(), 3, N, H, dh)
    g = torch.einsum("bihd,bjhd->bhij", k, k)
    g.diagonal(dim1=-2, dim2=-1).zero_()
    assert g.abs().max().item() <= 40
    for dh in (64, 88):
        for causal in (False, True):
            d = X.attn_selector(64, N, H, dh, causal, seed)
            assert X.selector_gap(d, 64, N, H, dh, causal) >= 64


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,dh", [(1, 64), (17, 64), (80, 88), (257, 64), (272, 88)])
def test_uniform_reference_and_sensitivity(N, dh, causal):
    B, H = 2, X.ATTN_H
    d = X.attn_uniform(B, N, H, dh, causal, 0)
    q, _, v = X.unpack_qkv(d["qkv"].float(), B, N, H, dh)
    assert q.abs().max().item() == 0 and set(v.unique().tolist()) <= {0.0, 1.0}
    ref = X.attention_ref(d["qkv"], B, N, H, dh, causal)
    assert (ref - d["ref"]).abs().max().item() < 1e-15
    assert torch.equal(d["keys"], torch.arange(1, N + 1) if causal else torch.full((N,), N))
    # one more copy of the last visible key (the clamped duplicate of row N - 1 left unmasked) turns count / keys into (count + 1) /
    # (keys + 1) in that key's column: far outside the bound wherever it changes anything (count < keys)
    rows = torch.arange(N)
    r = d["ref"].reshape(B, N, H, dh)[0, :, 0]                           # [N, dh]
    keys = d["keys"].double()
    col = (rows if causal else torch.full((N,), N - 1)) % dh
    have = r[rows, col]
    cnt = have * keys
    delta = ((cnt + 1) / (keys + 1) - have).abs()
    sees = cnt < keys - 0.5
    assert (delta[sees] > 4 * X.uniform_bound(have)[sees]).all() and (sees.any() or N == 1)
    assert (delta[sees] >= 0.19 * have[sees]).all()


@pytest.mark.parametrize("dh", [64, 88])
def test_isolation_logits(dh):
    B, N, H = 3, 81, X.ATTN_H
    d = X.attn_isolation(B, N, H, dh, False, 0)
    s = X.attention_logits(d["qkv"], B, N, H, dh)
    assert s.max().item() < -150 and s.min().item() > -250
    # a key of the neighbouring frame against this frame's queries: about +200
    q, k, _ = X.unpack_qkv(d["qkv"].double(), B, N, H, dh)
    cross = torch.einsum("bihd,bjhd->bhij", q[:-1], k[1:]) * dh ** -0.5
    assert cross.min().item() > 150
    cross = torch.einsum("bihd,bjhd->bhij", q[1:], k[:-1]) * dh ** -0.5
    assert cross.min().item() > 150


def test_random_family_has_a_small_and_a_large_column():
    B, N, H, dh = 3, 96, X.ATTN_H, 64
    d = X.attn_random(B, N, H, dh, True, 6.0)
    cm = X.column_max_admitted(d["qkv"], B, N, H, dh, True).reshape(B, N, H, dh)
    assert cm[:, -1, :, 1].min().item() > 64 and cm[:, -1, :, 2].max().item() < 0.1
    assert (cm[:, 1:] >= cm[:, :-1]).all()                               # causal: the visible set only grows
    full = X.column_max_admitted(d["qkv"], B, N, H, dh, False).reshape(B, N, H, dh)
    assert torch.equal(full[:, 0], cm[:, -1])


def test_attention_launcher_table_covers_every_instantiation():
    """The (variant, B, N) grid of test_gpu_attention_edges.py reaches every launcher instantiation of hirest_attention_bf16_rows."""
    reached = set()
    for dh in (64, 88):
        for causal in (False, True):
            for N in X.ATTN_N:
                for v in (1, 2, 7):
                    reached.add(X.attention_launcher(v, 3, N, dh, causal))
                if N > 80:
                    for v in (3, 4, 5, 6, 7):
                        reached.add(X.attention_launcher(v, 64, N, dh, causal))
    assert reached == X.attention_launchers_all()


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_attention_rejects_unsupported_shapes_before_any_launch(lib):
    """N = 273 and dh = 80 give HIREST_E_SHAPE for every variant: the entry returns before a launch, the placeholder pointers are never
    dereferenced."""
    X_PTR, SHAPE = 1 << 20, -2
    try:
        for variant in range(1, 8):
            assert lib.hirest_attention_select_kernel(variant) == 0
            for B in (3, 64):
                assert lib.hirest_attention_bf16(X_PTR, X_PTR, B, 273, 2, 64, 0.125, 0, None) == SHAPE
                assert lib.hirest_attention_bf16(X_PTR, X_PTR, B, 273, 2, 88, 0.1, 1, None) == SHAPE
                assert lib.hirest_attention_bf16(X_PTR, X_PTR, B, 96, 2, 80, 0.1, 0, None) == SHAPE
                assert lib.hirest_attention_bf16(X_PTR, X_PTR, B, 16, 2, 80, 0.1, 1, None) == SHAPE
                assert lib.hirest_attention_bf16_rows(X_PTR, X_PTR, B, 273, 2, 64, 0.125, 0, 1, None) == SHAPE
    finally:
        lib.hirest_attention_select_kernel(7)


def test_gemm_rejects_output_strides_the_epilogues_cannot_store_to(lib):
    """The epilogues store 4 (fp32) or 4 / 8 (bf16) consecutive elements per lane at out + m * ldo + n with n % 4 == 0: ldo % 4 != 0 would
    misalign them.  Rejected with HIREST_E_SHAPE before any launch."""
    from hirest_amd import _lib
    X_PTR = 1 << 20
    for epi in (_lib.EPI_BIAS_BF16, _lib.EPI_BIAS_GELU_BF16, _lib.EPI_BIAS_QGELU_BF16, _lib.EPI_BIAS_RESID_F32, _lib.EPI_BIAS_F32):
        for flags in (0, _lib.GEMM_REVERSE):
            for ldo in (133, 134, 135, 138):
                a = _lib.GemmArgs.make(X_PTR, 64, X_PTR, 64, None, X_PTR, ldo, 129, 132, 64, epi, None, 0, None, None, flags)
                assert lib.hirest_gemm_bf16(ctypes.byref(a), None) == -2, (epi, ldo)
    for epi in (_lib.EPI_BIAS_F32, _lib.EPI_BIAS_RESID_F32):             # the split-operand kernels share the fp32 epilogue
        a = _lib.GemmArgs.make(X_PTR, 64, X_PTR, 64, None, X_PTR, 134, 129, 132, 64, epi, None, 0, None, None, _lib.GEMM_X3)
        assert lib.hirest_gemm_bf16(ctypes.byref(a), None) == -2


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 GEMM family: tests/test_gpu_gemm_f32_exact.py
# ------------------------------------------------------------------------------------------------------------------------------
F32_SHAPES = sorted({s for _, _, _, _, shapes in X.F32_PLAIN for s in shapes} | {s for _, _, s in X.F32_ROWS})


@pytest.mark.parametrize("M,N,K", [s for s in F32_SHAPES if s[0] * s[1] * s[2] <= 1 << 26])
def test_f32_integer_inputs_are_exact_in_any_order(M, N, K):
    d = X.gemm_f32_exact(M, N, K)
    a, w, amax = d["a"], d["w"], d["amax"]
    assert amax == min(4095, (2 ** 24 - 1 - 24) // (15 * K)) and a.abs().max() == amax and w.abs().max() <= 15
    assert torch.equal(a, a.round()) and torch.equal(w, w.round())
    for t in (d["bias"], d["resid"], d["periodic"]):
        assert t.abs().max() <= 8 and torch.equal(t, t.round())
    assert d["periodic"].shape == (M + 3, N)
    # for every (m, n): sum_k |a| |w| + 24 < 2^24 — every partial sum of every summation order, and the epilogue's three addends on top
    worst = (a.abs().double() @ w.abs().double().t()).max().item()
    assert worst + 24 < X.F32_EXACT
    assert (a[0::16] == amax).all() and (w[0::8] >= 0).all() and (w[1::8] >= 0).all()
    if K >= 64:
        assert d["ref"].abs().max().item() > 0.25 * 15 * K * amax                      # the largest sums come near the bound
    assert torch.equal(d["ref"], d["ref"].float().double())
    if K <= 256:
        # 12 significant bits: an odd integer of magnitude >= 2048 changes when it is cut to an 11-bit significand
        v = a.abs().long()
        assert ((v >= 2048) & (v % 2 == 1)).any()


def test_f32_exact_bound_holds_for_the_shapes_too_large_to_multiply_here():
    """amax * 15 * K + 24 < 2^24 for every K in use: the precondition above without forming |a| |w|^T."""
    for _, _, K in F32_SHAPES + [(0, 0, k) for _, k, *_ in X.F32_OVERLAP]:
        assert X.f32_amax(K) >= 1 and X.f32_amax(K) * 15 * K + 24 < X.F32_EXACT


@pytest.mark.parametrize("M,N,K", [s for _, _, _, s in X.F32_ACT])
def test_f32_act_pre_activation_is_exact_and_in_range(M, N, K):
    d = X.gemm_f32_act(M, N, K)
    a, w, s = d["a"], d["w"], d["s"]
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set((w * 2.0 ** s).unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert torch.equal(d["bias"] * 8, (d["bias"] * 8).round()) and d["bias"].abs().max() <= 2
    # 8 * 2^s * x is an integer below 8 (K + 2 * 2^s) < 2^24: exact in fp32 in any order
    scaled = d["x"] * 8 * 2.0 ** s
    assert torch.equal(scaled, scaled.round()) and 8 * (K + 2 * 2 ** s) < X.F32_EXACT
    assert torch.equal(d["x"], d["x"].float().double())
    assert torch.equal((a @ w.t() + d["bias"]).double(), d["x"])
    x = d["x"]
    assert 1.0 < x.std().item() < 2.5 and (x.abs() <= 6).double().mean().item() > 0.99 and x.abs().max().item() < 12
    assert (x < -3).any() and (x > 3).any()
    for t in (d["resid"], d["periodic"]):
        assert t.abs().max() <= 8 and torch.equal(t, t.round())


@pytest.mark.parametrize("lda,K,M", sorted({(lda, K, M) for lda, K, M, *_ in X.F32_OVERLAP}))
def test_overlap_view_is_the_row_by_row_gather(lda, K, M):
    buf, off, g = X.overlap_view(M, lda, K)
    n = (M - 1) * lda + K
    assert off % 4 == 0 and lda % 4 == 0 and lda < K and off >= 4 * K and buf.numel() - off - n >= 4 * K
    assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + n:]).all()
    inner = buf[off:off + n]
    assert torch.equal(inner, inner.round()) and inner.abs().max() <= X.f32_amax(K)
    assert g.shape == (M, K) and torch.equal(torch.as_strided(buf, (M, K), (lda, 1), off), g)
    for m in (0, M // 2, M - 1):
        for k in (0, K - 1):
            assert g[m, k] == buf[off + m * lda + k]


def _f32_name(lib, entry, M, N, K, **fields):
    from hirest_amd import _lib
    fields = dict(dict(select_kernel=0, ring_mode=0, rows_ln_mode=2, cus=256), **fields)
    buf = ctypes.create_string_buffer(64)
    status = lib.hirest_gemm_f32_dispatch_name(ctypes.byref(_lib.GemmF32Query.make(entry, M, N, K, **fields)), buf, 64)
    return status, buf.value.decode()


def test_f32_shape_lists_reach_every_instantiation(lib):
    """With 256 CUs and the switch values the GPU test sets, every listed call takes the kernel it is listed under, and together the calls
    take every instantiation the fp32 dispatch can reach: when a threshold moves, a kernel cannot lose its test shapes unnoticed."""
    reached = set()
    for name, entry, M, N, K, fields in X.f32_dispatch_cases():
        assert _f32_name(lib, entry, M, N, K, **fields) == (0, name), (entry, M, N, K, fields)
        reached.add(name)
    assert sorted(reached) == X.F32_ALL_NAMES


def test_f32_dispatch_name_arguments(lib):
    from hirest_amd import _lib
    buf = ctypes.create_string_buffer(64)
    q = _lib.GemmF32Query.make("gemm", 64, 64, 64, cus=256)
    assert lib.hirest_gemm_f32_dispatch_name(ctypes.byref(q), buf, 64) == 0 and buf.value == b"m16<2,1,6>"   # -1 switches: the defaults
    assert lib.hirest_gemm_f32_dispatch_name(None, buf, 64) == -1 and lib.hirest_gemm_f32_dispatch_name(ctypes.byref(q), None, 64) == -1
    assert lib.hirest_gemm_f32_dispatch_name(ctypes.byref(q), buf, 47) == -1
    q.struct_size -= 4
    assert lib.hirest_gemm_f32_dispatch_name(ctypes.byref(q), buf, 64) == -1
    assert _f32_name(lib, "gemm", 64, 64, 0)[0] == -1 and _f32_name(lib, "gemm", 64, 64, 64, select_kernel=3)[0] == -1
    # shapes no kernel takes: the entry point's own status
    assert _f32_name(lib, "gemm", 64, 62, 64)[0] == -2 and _f32_name(lib, "gemm", 64, 64, 72)[0] == -2
    assert _f32_name(lib, "ln", 33, 8196, 512)[0] == -2 and _f32_name(lib, "ln", 16, 64, 1280)[0] == -2
    assert _f32_name(lib, "ln_colmax", 16, 4096, 768)[0] == -2 and _f32_name(lib, "rows_colmax", 64, 64, 512)[0] == -2
    assert _f32_name(lib, "layouts", 66, 64, 64, a_kmajor=1)[0] == -2
    # the ring threshold is the one decision of hirest_gemm_f32 itself that reads the CU count: 64 tiles per CU
    assert _f32_name(lib, "gemm", 64 * 128, 64 * 128, 64, cus=256) == (0, "ring<4>")
    assert _f32_name(lib, "gemm", 64 * 128, 64 * 127, 64, cus=256) == (0, "tile64")
    assert _f32_name(lib, "gemm", 64 * 128, 64 * 127, 64, cus=128) == (0, "ring<4>")
    assert _f32_name(lib, "gemm", 64 * 128, 64 * 128, 64, ring_mode=1) == (0, "tile64")
    # hirest_gemm_f32_ws without a usable workspace is hirest_gemm_f32
    assert _f32_name(lib, "ws", 300, 132, 1040, has_workspace=0) == (0, "tile64") and _f32_name(lib, "ws", 300, 132, 1040, has_workspace=1) == (0, "tile64.split")


def test_f32_gemm_rejects_strides_its_epilogue_cannot_use(lib):
    """out and resid are moved as 16-byte vectors at base + m * ld + n: ldo, ldr must be multiples of 4 and at least N; ln_out rows hold K
    floats.  HIREST_E_SHAPE before any launch: the placeholder pointers are never dereferenced."""
    P, SHAPE = 1 << 20, -2
    M, N, K = 64, 132, 256
    for ldo, ldr, resid in ((133, 132, None), (134, 132, None), (128, 132, None), (132, 133, P), (132, 134, P), (132, 128, P), (130, 132, P)):
        assert lib.hirest_gemm_f32(P, K, P, K, None, resid, ldr, None, 0, P, ldo, M, N, K, 0, None) == SHAPE, (ldo, ldr)
        assert lib.hirest_gemm_f32_ws(P, K, P, K, None, resid, ldr, None, 0, P, ldo, M, N, K, 0, None, 0, None) == SHAPE, (ldo, ldr)
        assert lib.hirest_gemm_f32_layouts(P, K, 0, P, K, 0, None, resid, ldr, P, ldo, M, N, K, 0, None, 0, None) == SHAPE, (ldo, ldr)
        assert lib.hirest_gemm_f32_ln(P, K, None, None, None, P, P, 1e-5, None, 0, P, K, None, resid, ldr, P, ldo, 16, N, K, 0, None) == SHAPE, (ldo, ldr)
    for ldl in (252, 255, 128):
        assert lib.hirest_gemm_f32_ln(P, K, None, None, None, P, P, 1e-5, P, ldl, P, K, None, None, 0, P, N, 16, N, K, 0, None) == SHAPE, ldl
    for ldo in (8197, 8198, 8192):
        assert lib.hirest_gemm_f32_ln_colmax(P, 768, P, P, 1e-5, P, 768, None, P, ldo, P, 16, 8196, 768, None) == SHAPE, ldo


# ------------------------------------------------------------------------------------------------------------------------------
# split-operand attention: tests/test_gpu_attention_x3_exact.py
# ------------------------------------------------------------------------------------------------------------------------------
X3A_SEL_DH = [dh for dh in X.X3A_DH if dh >= 32]
# the generators are the same code for every shape: the host side takes two tiles with a ragged end, the first fetch at k0 + 64, Tq < Tk
# with ten tiles and Tq > Tk, over the narrowest, the widest and the two padded head widths
X3A_HOST = [(3, 31, 33, 2, 32), (1, 64, 65, 3, 36), (3, 129, 97, 2, 68), (1, 33, 289, 3, 88), (3, 289, 33, 2, 96), (1, 97, 64, 2, 64)]
x3a_host = pytest.mark.parametrize("B,Tq,Tk,H,dh", X3A_HOST, ids=[X.x3a_id(c) for c in X3A_HOST])


def test_x3a_cases_cover_every_axis_value():
    for dhs in (X.X3A_DH, X3A_SEL_DH):
        cases = X.x3a_cases(dhs)
        assert {(Tq, Tk) for _, Tq, Tk, _, _ in cases} == set(X.X3A_SHAPES) and len(cases) == 2 * len(X.X3A_SHAPES)
        assert {c[4] for c in cases} == set(dhs) and {c[0] for c in cases} == set(X.X3A_B) and {c[3] for c in cases} == set(X.X3A_H)
        for axis, values in ((0, X.X3A_B), (3, X.X3A_H)):                  # both B and both H against more than one head width and shape
            for val in values:
                assert len({c[4] for c in cases if c[axis] == val}) >= 3 and len({c[1:3] for c in cases if c[axis] == val}) >= 4
        for shape in X.X3A_SHAPES:                                         # every shape with both batch sizes and two head widths
            mine = [c for c in cases if c[1:3] == shape]
            assert {c[0] for c in mine} == set(X.X3A_B) and len({c[4] for c in mine}) == 2
    assert any(Tq == Tk for Tq, Tk in X.X3A_SHAPES)                     # the packed layout has cases


@pytest.mark.parametrize("frac_in_k", [True, False], ids=["klo", "qlo"])
@x3a_host
def test_x3_selector_preconditions(B, Tq, Tk, H, dh, frac_in_k):
    d = (X.x3_selector_klo if frac_in_k else X.x3_selector_qlo)(B, Tq, Tk, H, dh)
    q, k, v, pi, c, s = d["q"], d["k"], d["v"], d["pi"], d["c"], d["s"]
    assert q.shape == (B, Tq, H, dh) and k.shape == v.shape == (B, Tk, H, dh) and q.dtype == k.dtype == v.dtype == torch.float32
    gap = X.x3_selector_gap(d)
    print(f"c = 2^{math.log2(c):.0f}, gap {gap:.1f}")
    assert gap >= X.X3A_GAP and c == 2.0 ** round(math.log2(c)) and X.x3_selector_gap(dict(d, q=q / 2)) < X.X3A_GAP   # the smallest such c
    # s: balanced +-1, pairwise distinct within a (frame, head)
    assert set(s.unique().tolist()) == {-1.0, 1.0} and (s.sum(-1) == 0).all()
    for b in range(B):
        for h in range(H):
            assert torch.unique(s[b, :, h], dim=0).shape[0] == Tk
    # pi: every key when Tq >= Tk; key Tk - 1 and one key of every 32-key tile always
    assert pi.shape == (B, H, Tq) and pi.min() >= 0 and pi.max() < Tk
    for row in pi.reshape(B * H, Tq):
        hit = set(row.tolist())
        assert Tk - 1 in hit and {j // 32 for j in hit} == set(range((Tk + 31) // 32)) and (Tq < Tk or len(hit) == Tk)
    # hi and lo parts exactly as stated
    sel = torch.gather(s, 1, pi.permute(0, 2, 1)[..., None].expand(B, Tq, H, dh))
    (qh, ql), (kh, kl) = X.hi_lo(q), X.hi_lo(k)
    if frac_in_k:
        assert torch.equal(kh, torch.ones_like(k)) and torch.equal(kl, X.X3A_FRAC * s) and torch.equal(qh, c * sel) and (ql == 0).all()
    else:
        assert torch.equal(qh, torch.full_like(q, c)) and torch.equal(ql, c * X.X3A_FRAC * sel) and torch.equal(kh, s) and (kl == 0).all()
    assert torch.equal(qh + ql, q) and torch.equal(kh + kl, k)
    # every partial sum is a multiple of c 2^-10 below 2^24 of it: the sum of the magnitudes of all three products' terms
    unit = c * X.X3A_FRAC
    assert torch.equal(q / unit, (q / unit).round()) and dh * (1 + 2 * X.X3A_FRAC) / X.X3A_FRAC < X.F32_EXACT
    # V: 16-bit significands, exponent in {-1, 0, 1}, v == hi + lo with the lo part alive; no two rows agree
    vh, vl = X.hi_lo(v)
    assert torch.equal(vh + vl, v) and (v.view(torch.int32) & 0xFF == 0).all() and (vl != 0).float().mean().item() > 0.9
    assert v.abs().min().item() >= 0.5 and v.abs().max().item() < 4.0
    assert torch.unique(v.reshape(-1, dh), dim=0).shape[0] == B * Tk * H
    # the fp64 reference puts everything on pi(i)
    assert torch.equal(X.attention_x3_ref(q, k, v).float(), d["want"])


@pytest.mark.parametrize("frac_in_k", [True, False], ids=["klo", "qlo"])
@x3a_host
def test_x3_selector_emulation_needs_its_cross_term(B, Tq, Tk, H, dh, frac_in_k):
    """The fp32 emulation of the kernel returns the selected V rows bit for bit, and does not once the score term that carries the selection
    (k_lo q_hi for klo, k_hi q_lo for qlo) or the v_lo p_hi term is left out; the other cross term is zero in that family."""
    d = (X.x3_selector_klo if frac_in_k else X.x3_selector_qlo)(B, Tq, Tk, H, dh)
    q, k, v, want = d["q"], d["k"], d["v"], d["want"]
    assert torch.equal(X.attention_x3_emulated(q, k, v).view(torch.int32), want.view(torch.int32))
    carrying, idle = ("klqh", "khql") if frac_in_k else ("khql", "klqh")
    assert not torch.equal(X.attention_x3_emulated(q, k, v, drop=(carrying,)), want)
    assert torch.equal(X.attention_x3_emulated(q, k, v, drop=(idle,)), want)
    assert not torch.equal(X.attention_x3_emulated(q, k, v, drop=("vlph",)), want)
    assert torch.equal(X.attention_x3_emulated(q, k, v, drop=("vhpl",)), want)               # (p is 0 or 1: no lo part)


@pytest.mark.parametrize("B,Tq,Tk,H,dh", X3A_HOST + [(1, 1, 1, 2, 4), (3, 33, 31, 3, 4)])
def test_x3_uniform_bound_under_the_emulation(B, Tq, Tk, H, dh):
    d = X.x3_uniform(B, Tq, Tk, H, dh)
    assert d["q"].abs().max().item() == 0 and set(d["v"].unique().tolist()) <= {0.0, 1.0}
    ref = d["ref"]
    assert (X.attention_x3_ref(d["q"], d["k"], d["v"]) - ref).abs().max().item() < 1e-15
    count = ref[0, 0, 0] * Tk
    assert torch.equal(count.round(), torch.tensor([len(range(c, Tk, dh)) for c in range(dh)], dtype=torch.float64)) and count.sum().round() == Tk
    err = (X.attention_x3_emulated(d["q"], d["k"], d["v"]).double() - ref).abs()
    assert (err <= d["bound"]).all()
    # one key too many (the clamped copy of key Tk - 1 left unmasked) or too few (key Tk - 1 masked away)
    have = ref[0, 0, 0, (Tk - 1) % dh]
    for wrong in ((have * Tk + 1) / (Tk + 1), (have * Tk - 1) / max(Tk - 1, 1)):
        assert abs(wrong - have) > 1000 * have * 2.0 ** -22 or Tk == 1


def test_x3_isolation_logits():
    B, Tq, Tk, H, dh = 3, 33, 65, 2, 36
    d = X.x3_isolation(B, Tq, Tk, H, dh)
    s = X.attention_x3_logits(d["q"], d["k"])
    assert s.max().item() < -150 and s.min().item() > -250
    for qa, kb in ((d["q"][:-1], d["k"][1:]), (d["q"][1:], d["k"][:-1])):          # a key of the neighbouring frame: about +200
        assert X.attention_x3_logits(qa, kb).min().item() > 150


@pytest.mark.parametrize("qscale", [1, 3, 6])
def test_x3_random_family_and_the_restatement(qscale):
    """The restatement is the reference when every lo part is zero: bit for bit with one key (p = 1), and with many keys up to the lo x lo
    term of p's split alone (bf16-valued q, k, v do not make p bf16-valued), far below the family's own Y.  The fp32 emulation stays within
    the factor 2 of Y that the GPU test allows the kernel."""
    B, Tq, Tk, H, dh = 3, 33, 97, 2, 36
    d = X.x3_random(B, Tq, Tk, H, dh, qscale)
    q, k, v = d["q"], d["k"], d["v"]
    cm = X.x3_column_max(v)
    assert cm[:, :, :, 1].min().item() > 64 and cm[:, :, :, 2].max().item() < 0.1 and (X.hi_lo(k)[1] != 0).float().mean().item() > 0.9
    import _whisper_enc_ref as W
    heads = lambda t: t.double().permute(0, 2, 1, 3)
    unsplit = W.attention_heads(heads(q), heads(k), heads(v), False).permute(0, 2, 1, 3)            # (exp / sum against torch.softmax)
    assert ((unsplit - X.attention_x3_ref(q, k, v)).abs() / cm).max().item() < 1e-14
    # lo parts zero: one-key softmax (p = 1, no lo part either) makes the restatement the reference bit for bit
    q1, k1, v1 = (t.to(torch.bfloat16).float() for t in (q, k[:, :1], v[:, :1]))
    assert torch.equal(X.attention_x3_restated(q1, k1, v1), X.attention_x3_ref(q1, k1, v1))
    # and with many keys only p's lo x lo term (2^-18 relative) separates them
    qb, kb, vb = (t.to(torch.bfloat16).float() for t in (q, k, v))
    e0 = ((X.attention_x3_restated(qb, kb, vb) - X.attention_x3_ref(qb, kb, vb)).abs() / cm).max().item()
    Y = ((X.attention_x3_restated(q, k, v) - X.attention_x3_ref(q, k, v)).abs() / cm).max().item()
    E = ((X.attention_x3_emulated(q, k, v).double() - X.attention_x3_ref(q, k, v)).abs() / cm).max().item()
    R = ((X.attention_x3_emulated(q, k, v).double() - X.attention_x3_restated(q, k, v)).abs() / cm).max().item()
    print(f"qscale {qscale}: lo-free restatement {e0:.2e}, Y {Y:.2e}, emulation / Y {E / Y:.2f}, emulation - restatement {R:.2e}")
    assert e0 < 2.0 ** -17 and e0 < Y / 2 and E <= 2 * Y
