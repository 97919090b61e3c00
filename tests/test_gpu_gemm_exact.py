"""The bf16 GEMM kernels (csrc/gemm.hip, csrc/gemm_shared.h) held to the bit at tile-edge shapes.

Operands are small integers (tests/_exact_inputs.py; preconditions in tests/test_exact_inputs_host.py), so every partial sum of the
fp32 accumulation is exact in any order: the expected output of every selectable kernel, tile walk, split-K order and of the
split-operand ("x3") kernels is one bit pattern, compared with torch.equal on the integer view.  Only the GELU epilogues are not
exact; they are held per element to half a bf16 ulp plus twice the fp32 error csrc/common.h documents for gelu_erf.

Every call builds its own hirest_gemm_args (strides and flags included), asks hirest_gemm_dispatch_name first and asserts the
instantiation it means to test, so a case never silently runs another kernel."""
import ctypes as C

import pytest
import torch

import _exact_inputs as X

pytestmark = pytest.mark.gpu

SENT32 = 0x4B1DE5A5          # fp32 sentinel bits (a finite value no exact result equals)
SENT16 = 0x5A5B              # bf16 sentinel bits
GUARD_ROWS = 3

KERNEL_NAMES = {1: "gemm_t128<%d>", 2: "gemm_t256<%d, 4>", 3: "gemm_t256<%d, 5>", 4: "gemm_t256p<%d>", 5: "gemm_t256q<%d>",
                6: "gemm_p256<%d, 64, false, 1>", 7: "gemm_p256<%d, 128, false, 1>", 8: "gemm_pp256<%d, 1>", 9: "gemm_pq256<%d>"}
KERNEL_IDS = ["auto", "t128", "t256x4", "t256x5", "t256p", "t256q", "p256w8", "p256w4", "pp256", "pq256"]


def expected_kernel(kernel, epi, M, N):
    """The instantiation hirest_gemm_select_kernel(kernel) means for a plain epilogue (include/hirest_hip.h)."""
    if kernel == 0:
        big = M * N >= 2048 * 1024 and M >= 512 and N >= 256
        return ("gemm_pq256<%d>" if big else "gemm_t128<%d>") % epi
    return KERNEL_NAMES[kernel] % epi


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib
    return _lib.load()


@pytest.fixture(params=list(range(10)), ids=KERNEL_IDS)
def kernel(request):
    from hirest_amd import ops
    ops.gemm_select_kernel(request.param)
    try:
        yield request.param
    finally:
        ops.gemm_select_kernel(0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _gemm(lib, expect, a, lda, w, ldw, bias, out, ldo, M, N, K, epi, pos=None, P=0, aux0=None, aux1=None, flags=0):
    """hirest_gemm_bf16 as ops.gemm calls it, with every stride and flag in the caller's hands; `expect` is the instantiation the
    dispatch must name for it."""
    from hirest_amd import _lib, ops
    args = _lib.GemmArgs.make(_ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(out), ldo, M, N, K, epi, _ptr(pos), P, _ptr(aux0), _ptr(aux1), int(flags))
    name = C.create_string_buffer(64)
    _lib.check(lib.hirest_gemm_dispatch_name(C.byref(args), name, 64), "hirest_gemm_dispatch_name")
    assert name.value.decode() == expect
    _lib.check(lib.hirest_gemm_bf16(C.byref(args), ops.stream_ptr()), "hirest_gemm_bf16")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))


def _sentinel(shape, dtype, dev):
    if dtype == torch.float32:
        return torch.full(shape, SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)


_DEV_CACHE = {}


def _data(M, N, K, dev):
    """The exact inputs of a shape and every expected output, on the device; computed once per shape (the last shape is kept)."""
    key = (M, N, K)
    if key not in _DEV_CACHE:
        _DEV_CACHE.clear()
        d = X.gemm_exact(M, N, K)
        P, B = d["P"], M // d["P"]
        ref = d["ref"] + 0.0
        lin = ref + d["bias"]
        patch = (lin.reshape(B, P, N) + d["pos"][1:]).reshape(M, N)
        e = {k: d[k].to(dev) for k in ("a", "w", "bias", "resid", "pos")}
        e.update(P=P, B=B, ref=ref.to(dev), lin=lin.to(dev), lin_bf16=lin.to(torch.bfloat16).to(dev), res=(d["resid"] + lin).to(dev),
                 patch=patch.to(dev))
        _DEV_CACHE[key] = e
    return _DEV_CACHE[key]


def _run_exact_epilogues(lib, dev, d, kernel, M, N, K, pad_a=0, pad_w=0, pad_o=0, flags=0, name=expected_kernel):
    """Every exact epilogue of one kernel on one shape.  With padding, the operands' pad columns hold NaN and the output buffer's pad columns
    and GUARD_ROWS rows after the last one hold a sentinel that must survive."""
    from hirest_amd import _lib
    lda, ldw, ldo = K + pad_a, K + pad_w, N + pad_o
    a = torch.full((M, lda), float("nan"), dtype=torch.bfloat16, device=dev); a[:, :K] = d["a"]
    w = torch.full((N, ldw), float("nan"), dtype=torch.bfloat16, device=dev); w[:, :K] = d["w"]

    def run(epi, dtype, want, bias=d["bias"], init=None, rows=M, row_of=None, **kw):
        buf = _sentinel((rows + GUARD_ROWS, ldo), dtype, dev)
        if init is not None:
            buf[:M, :N] = init
        exp = buf.clone()
        if row_of is None:
            exp[:M, :N] = want
        else:
            exp[row_of, :N] = want
        _gemm(lib, name(kernel, epi, M, N), a, lda, w, ldw, bias, buf, ldo, M, N, K, epi, flags=flags, **kw)
        assert _same_bits(buf, exp), (kernel, epi, M, N, K)

    run(_lib.EPI_BIAS_F32, torch.float32, d["lin"])
    run(_lib.EPI_BIAS_F32, torch.float32, d["ref"], bias=None)
    run(_lib.EPI_BIAS_RESID_F32, torch.float32, d["res"], init=d["resid"])
    run(_lib.EPI_BIAS_BF16, torch.bfloat16, d["lin_bf16"])            # round to nearest even: the data holds exact ties (host test)
    # patch embedding: row b * P + p lands in row b * (P + 1) + 1 + p with pos[1 + p] added; the CLS rows b * (P + 1) keep their sentinel
    P, B = d["P"], d["B"]
    rows = torch.arange(M, device=dev)
    run(_lib.EPI_PATCH_POS_F32, torch.float32, d["patch"], rows=B * (P + 1), row_of=rows + rows // P + 1, pos=d["pos"], P=P)


@pytest.mark.parametrize("M,N,K", X.GEMM_SHAPES)
def test_exact_epilogues_at_tile_edges(dev, lib, kernel, M, N, K):
    _run_exact_epilogues(lib, dev, _data(M, N, K, dev), kernel, M, N, K)


@pytest.mark.parametrize("M,N,K", X.GEMM_STRIDED_SHAPES)
def test_strides_and_untouched_memory(dev, lib, kernel, M, N, K):
    """lda = K + 8, ldw = K + 16, ldo = N + 8 (the alignment residue ldo = N already has): the NaN in the operands' padding is never
    multiplied in, and the output's padding columns and the rows after M - 1 are bit-unchanged."""
    _run_exact_epilogues(lib, dev, _data(M, N, K, dev), kernel, M, N, K, pad_a=8, pad_w=16, pad_o=8)


@pytest.mark.parametrize("k", [6, 8, 9], ids=["p256w8", "pp256", "pq256"])
def test_reverse_walk_is_exact(dev, lib, k):
    """HIREST_GEMM_REVERSE on more tiles than CUs: the backward tile walk gives the exact reference, hence the forward walk's bits."""
    from hirest_amd import _lib, ops
    M, N, K = X.GEMM_BIG
    ops.gemm_select_kernel(k)
    try:
        _run_exact_epilogues(lib, dev, _data(M, N, K, dev), k, M, N, K, flags=_lib.GEMM_REVERSE)
    finally:
        ops.gemm_select_kernel(0)


@pytest.mark.parametrize("word", [8, 16, 32, 48])
@pytest.mark.parametrize("k", [0, 6], ids=["auto", "p256w8"])
def test_debug_tile_orders_are_exact(dev, lib, k, word):
    """hirest_gemm_debug_mode bits 3-5 (grouped / panel-major / paired edge units) reorder the persistent kernel's tile walk: every
    tile is still computed once, so the result is the exact reference, not merely "equal to the default order"."""
    from hirest_amd import _lib, ops
    M, N, K = X.GEMM_BIG
    d = _data(M, N, K, dev)

    def name(kernel, epi, M, N):      # the three tower epilogues have the instantiation that reads the word; the others ignore it
        if epi in (_lib.EPI_BIAS_BF16, _lib.EPI_BIAS_GELU_BF16, _lib.EPI_BIAS_RESID_F32):
            return "gemm_p256<%d, 64, true, 1>" % epi
        return expected_kernel(kernel, epi, M, N)

    ops.gemm_select_kernel(k)
    try:
        lib.hirest_gemm_debug_mode(word)
        _run_exact_epilogues(lib, dev, d, k, M, N, K, name=name)
        _run_exact_epilogues(lib, dev, d, k, M, N, K, flags=_lib.GEMM_REVERSE, name=name)
    finally:
        lib.hirest_gemm_debug_mode(0)
        ops.gemm_select_kernel(0)


@pytest.mark.parametrize("M,N,K", X.GEMM_GELU_SHAPES)
def test_gelu_epilogues_per_element(dev, lib, kernel, M, N, K):
    """GELU / QuickGELU of an exact pre-activation against x Phi(x) / x sigmoid(1.702 x) in fp64, per element:
    |out - g| <= ulp_bf16(g) / 2 + 4e-5 |g| + 2e-6 (X.gelu_bound).
    Worst error / bound observed on the MI355X, the same for all ten selections and both shapes: GELU 0.963, QuickGELU 0.958 — all of it the
    half ulp of the bf16 store; no element exceeds half an ulp, so the fp32 terms are not drawn on at all."""
    from hirest_amd import _lib
    d = X.gemm_gelu(M, N, K)
    a, w, bias = d["a"].to(dev), d["w"].to(dev), d["bias"].to(dev)
    for epi, ref in ((_lib.EPI_BIAS_GELU_BF16, X.gelu_ref), (_lib.EPI_BIAS_QGELU_BF16, X.qgelu_ref)):
        out = _sentinel((M + GUARD_ROWS, N), torch.bfloat16, dev)
        _gemm(lib, expected_kernel(kernel, epi, M, N), a, K, w, K, bias, out, N, M, N, K, epi)
        g = ref(d["x"])
        got = out[:M].cpu().double()
        assert torch.isfinite(got).all()
        ratio = ((got - g).abs() / X.gelu_bound(g)).max().item()
        fp32_part = (((got - g).abs() - X.ulp_bf16(g) / 2).clamp(min=0) / (4e-5 * g.abs() + 2e-6)).max().item()
        print(f"gelu epilogue {epi} kernel {kernel} {M}x{N}x{K}: worst error / bound {ratio:.4f}; error beyond half an ulp / fp32 terms {fp32_part:.4f}")
        assert ratio <= 1.0
        assert _same_bits(out[M:], _sentinel((GUARD_ROWS, N), torch.bfloat16, dev))


# ------------------------------------------------------------------------------------------------------------------------------
# split-operand kernels (HIREST_GEMM_X3)
# ------------------------------------------------------------------------------------------------------------------------------
def _x3_cases():
    from hirest_amd import _lib
    x3, t128 = _lib.GEMM_X3, _lib.GEMM_X3 | _lib.GEMM_X3_T128
    return [("gemm_t128x3<%d, 2>", (131, 132, 64), x3, 0), ("gemm_t128x3<%d, 2>", (1, 4, 32), x3, 0),
            ("gemm_t128x3<%d, 3>", (2060, 2048, 32), t128, 0), ("gemm_pp256x3<%d>", (4360, 4100, 32), x3, 0),
            ("gemm_pq256x3<%d>", (4360, 4100, 32), x3, 9)]


@pytest.mark.parametrize("frac_in_a", [True, False], ids=["a_hi_lo", "w_hi_lo"])
@pytest.mark.parametrize("case", range(5), ids=["t128x3_w2", "t128x3_w2_one_row", "t128x3_w3", "pp256x3", "pq256x3"])
def test_x3_kernels_exact(dev, lib, case, frac_in_a):
    """A W^T from split operands built on the CPU: one operand is integer + integer * 2^-10 (hi and lo parts), the other integer (lo = 0,
    so the lo * lo product the kernel drops is 0).  Run with the fraction in A, then in W: the hi-lo and the lo-hi product paths."""
    from hirest_amd import _lib, ops
    fmt, (M, N, K), flags, sel = _x3_cases()[case]
    d = X.gemm_x3(M, N, K, frac_in_a)
    a2, w2, bias = d["a2"].to(dev), d["w2"].to(dev), d["bias"].to(dev)
    lin = (d["ref"] + 0.0 + d["bias"]).to(dev)
    ops.gemm_select_kernel(sel)
    try:
        out = _sentinel((M + GUARD_ROWS, N), torch.float32, dev)
        exp = out.clone(); exp[:M] = lin
        _gemm(lib, fmt % _lib.EPI_BIAS_F32, a2, 2 * K, w2, 2 * K, bias, out, N, M, N, 2 * K, _lib.EPI_BIAS_F32, flags=flags)
        assert _same_bits(out, exp)
        out = _sentinel((M + GUARD_ROWS, N), torch.float32, dev)
        out[:M] = d["resid"].to(dev)
        exp = out.clone(); exp[:M] = (d["resid"] + (d["ref"] + d["bias"])).to(dev)
        _gemm(lib, fmt % _lib.EPI_BIAS_RESID_F32, a2, 2 * K, w2, 2 * K, bias, out, N, M, N, 2 * K, _lib.EPI_BIAS_RESID_F32, flags=flags)
        assert _same_bits(out, exp)
    finally:
        ops.gemm_select_kernel(0)


@pytest.mark.parametrize("frac_in_a", [True, False], ids=["a_hi_lo", "w_hi_lo"])
def test_x3_split_k_exact(dev, lib, frac_in_a):
    """HIREST_EPI_BIAS_RESID_F32 with scratch in aux0 (4 M N floats, as csrc/joint_x3.hip sizes it): 9 tiles of 16 steps are cut into two K
    slices.  The split shows in the scratch — exactly two of its four planes are written and they add up to the product — and the
    result is the exact reference."""
    from hirest_amd import _lib
    M, N, K = 300, 260, 512
    d = X.gemm_x3(M, N, K, frac_in_a)
    a2, w2, bias = d["a2"].to(dev), d["w2"].to(dev), d["bias"].to(dev)
    scratch = _sentinel((4, M, N), torch.float32, dev)
    out = _sentinel((M + GUARD_ROWS, N), torch.float32, dev)
    out[:M] = d["resid"].to(dev)
    exp = out.clone(); exp[:M] = (d["resid"] + (d["ref"] + d["bias"])).to(dev)
    _gemm(lib, "gemm_t128x3<%d, 2>" % _lib.EPI_BIAS_RESID_F32, a2, 2 * K, w2, 2 * K, bias, out, N, M, N, 2 * K, _lib.EPI_BIAS_RESID_F32,
          aux0=scratch, flags=_lib.GEMM_X3 | _lib.GEMM_X3_T128)
    assert _same_bits(out, exp)
    assert not (_bits(scratch[:2]) == SENT32).any()
    assert _same_bits(scratch[2:], _sentinel((2, M, N), torch.float32, dev))
    assert torch.equal(scratch[0] + scratch[1], d["ref"].to(dev) + 0.0)
    half = (d["a"][:, :K // 2].double() @ d["w"][:, :K // 2].double().t()).float().to(dev)
    assert torch.equal(scratch[0], half + 0.0)                      # slice 0 is the first half of the K range


@pytest.mark.parametrize("sel,flags_t128,fmt", [(0, False, "gemm_pp256x3<9>"), (9, False, "gemm_pq256x3<9>"), (0, True, "gemm_t128x3<9, 2>")],
                         ids=["pp256x3", "pq256x3", "t128x3"])
def test_x3_gelu_split2_epilogue(dev, lib, sel, flags_t128, fmt):
    """HIREST_EPI_BIAS_GELU_SPLIT2 on an exact pre-activation: every hi is the bf16 rounding of hi + lo, and
    |hi + lo - g| <= 4e-5 |g| + 2e-6 + 2^-17 |g| (the fp32 GELU terms of X.gelu_bound and the 16 significand bits of a split value);
    the padding beyond 2 N is untouched.  Worst error / bound observed on the MI355X: 0.150 for all three kernels."""
    from hirest_amd import _lib, ops
    M, N, K = X.X3_GELU_SHAPE
    d = X.gemm_x3_gelu(M, N, K)
    a2, w2, bias = d["a2"].to(dev), d["w2"].to(dev), d["bias"].to(dev)
    ldo = 2 * N + 8
    out = _sentinel((M + GUARD_ROWS, ldo), torch.bfloat16, dev)
    ops.gemm_select_kernel(sel)
    try:
        _gemm(lib, fmt, a2, 2 * K, w2, 2 * K, bias, out, ldo, M, N, 2 * K, _lib.EPI_BIAS_GELU_SPLIT2,
              flags=_lib.GEMM_X3 | (_lib.GEMM_X3_T128 if flags_t128 else 0))
    finally:
        ops.gemm_select_kernel(0)
    assert _same_bits(out[:M, 2 * N:], _sentinel((M, 8), torch.bfloat16, dev)) and _same_bits(out[M:], _sentinel((GUARD_ROWS, ldo), torch.bfloat16, dev))
    got = out[:M, :2 * N].cpu().reshape(M, N // 32, 2, 32)
    hi, lo = got[:, :, 0].reshape(M, N), got[:, :, 1].reshape(M, N)
    both = hi.float() + lo.float()
    assert torch.equal(both.double(), hi.double() + lo.double())                       # (the fp32 sum is exact)
    assert _same_bits(both.to(torch.bfloat16), hi)
    g = X.gelu_ref(d["x"])
    ratio = ((both.double() - g).abs() / (4e-5 * g.abs() + 2e-6 + 2.0 ** -17 * g.abs())).max().item()
    print(f"gelu + split epilogue {fmt}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# fused LN-statistics producer
# ------------------------------------------------------------------------------------------------------------------------------
def _finalize(part, rows, D, eps, dev):      # as tests/test_gpu_lnfold.py reads the partials
    from hirest_amd import _lib, ops
    stats = torch.empty((rows, 2), device=dev)
    _lib.check(_lib.load().hirest_ln_stats_finalize(part.data_ptr(), part.shape[1], stats.data_ptr(), eps, rows, D, None, ops.stream_ptr()),
               "hirest_ln_stats_finalize")
    return stats


@pytest.mark.parametrize("sel,fmt", [(0, "gemm_pq256<6>"), (6, "gemm_p256<6, 64, false, 1>"), (8, "gemm_pp256<6, 1>"), (9, "gemm_pq256<6>")],
                         ids=["auto", "p256w8", "pp256", "pq256"])
@pytest.mark.parametrize("M,N,K", X.GEMM_LNSTATS_SHAPES)
def test_lnstats_producer_exact(dev, lib, sel, fmt, M, N, K):
    """HIREST_EPI_BIAS_RESID_LNSTATS_F32 at its smallest accepted shape and at a ragged one: the residual stream is resid + a w^T + bias
    to the bit, the bf16 copy is its RNE rounding, and the per-group partials are the exact integer sums of x and x^2 over the rounded
    values (all below 2^24: host test), so the finalized (mean, rstd) are the exact row sums' within fp32 rounding."""
    from hirest_amd import _lib, ops
    c = X.gemm_lnstats(M, N, K)
    d = {k: c[k].to(dev) for k in ("a", "w", "bias", "resid")}
    d["res"] = (c["resid"] + (c["ref"] + c["bias"])).to(dev)
    G = (N + 63) // 64
    out = _sentinel((M + GUARD_ROWS, N), torch.float32, dev)
    out[:M] = d["resid"]
    exp = out.clone(); exp[:M] = d["res"]
    xb = _sentinel((M + GUARD_ROWS, N), torch.bfloat16, dev)
    part = torch.full((M, G, 2), float("nan"), device=dev)
    ops.gemm_select_kernel(sel)
    try:
        _gemm(lib, fmt, d["a"], K, d["w"], K, d["bias"], out, N, M, N, K, _lib.EPI_BIAS_RESID_LNSTATS_F32, aux0=xb, aux1=part)
    finally:
        ops.gemm_select_kernel(0)
    assert _same_bits(out, exp)
    want_xb = d["res"].to(torch.bfloat16)
    assert _same_bits(xb[:M], want_xb) and _same_bits(xb[M:], _sentinel((GUARD_ROWS, N), torch.bfloat16, dev))
    f = torch.zeros((M, G * 64), dtype=torch.float64, device=dev); f[:, :N] = want_xb.double()
    want = torch.stack([f.reshape(M, G, 64).sum(-1), (f * f).reshape(M, G, 64).sum(-1)], dim=-1)
    assert torch.equal(part.double(), want)                                            # integer sums: exact in any order
    eps = torch.tensor(1e-6, dtype=torch.float32).item()                               # the fp32 eps the entry receives, as a double
    stats = _finalize(part, M, N, eps, dev).double()
    s1, s2 = want[..., 0].sum(1), want[..., 1].sum(1)                                  # the exact row sums of x and x^2
    mean = s1 / N
    var = s2 / N - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps)
    # hirest_ln_stats_finalize adds the partials and forms mean, var and rstd in fp64 (csrc/elementwise.hip: ln_finalize_kernel), so from exact
    # partials each result is the fp32 rounding of the fp64 value: 2^-24 relative; rstd gets a second 2^-24 for the fp64 roundings behind it
    # (var = Q / D - mean^2 cancels at most to var / E x^2 >= 2^-20 here).  Worst error / bound observed on the MI355X: mean 0.876, rstd 0.447
    mean_ratio = ((stats[:, 0] - mean).abs() / (2.0 ** -24 * mean.abs() + 1e-300)).max().item()
    rstd_ratio = (((stats[:, 1] - rstd) / rstd).abs() / (2 * 2.0 ** -24)).max().item()
    print(f"lnstats {fmt} {M}x{N}x{K}: worst mean error / bound {mean_ratio:.4f}, rstd error / bound {rstd_ratio:.4f}")
    assert mean_ratio <= 1.0 and rstd_ratio <= 1.0
