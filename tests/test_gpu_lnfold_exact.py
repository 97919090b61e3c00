"""The LN-fold consumer epilogues (HIREST_EPI_LNFOLD_BF16 / _GELU_BF16; csrc/gemm_shared.h) of the ping-pong kernels held to the bit at tile edges.

out = acc * rstd + (s * (-mean * rstd) + b') with acc = a w^T.  a, w, b' are the small integers of tests/_exact_inputs.py (gemm_exact), s the
integer row sums of w, mean an integer in [-4, 4] and rstd one of 0.5, 1, 2: every intermediate is an integer or a half-integer far below
2^23, exact in fp32 in any order and with or without fused multiply-adds, so the expected output is ONE bit pattern — the exact value rounded to
bf16 once (round to nearest even; the data holds ties) — compared with torch.equal on the int16 view.  fold_exact() asserts these preconditions
on the CPU for every shape it is used with.  Only the GELU form is not exact; it is held per element to _exact_inputs.gelu_bound.

Every call builds its own hirest_gemm_args, asks hirest_gemm_dispatch_name first and asserts the instantiation it means to test."""
import ctypes as C

import numpy as np
import pytest
import torch

import _exact_inputs as X

pytestmark = pytest.mark.gpu

SENT16 = 0x5A5B              # bf16 sentinel bits
GUARD_ROWS = 3
EPI_FOLD, EPI_FOLD_GELU = 7, 8
# hirest_gemm_select_kernel value -> the instantiation it means for the fold consumers (0: automatic = pq256)
KERNELS = {0: "gemm_pq256<%d>", 8: "gemm_pp256<%d, 1>", 9: "gemm_pq256<%d>"}
KERNEL_IDS = {0: "auto", 8: "pp256", 9: "pq256"}
# (M, N, K); the contract of the fold epilogues is M >= 64, N >= 256, N % 4 == 0
SHAPES = [(64, 256, 64),          # smallest accepted shape
          (129, 264, 192),        # last 64-column group 8 columns wide
          (257, 260, 192),        # N % 8 == 4: the 8-byte store; M one row past a panel
          (255, 316, 192),        # 60-column last group: seven 16-byte chunks and one 8-byte
          (385, 644, 128),        # three column tiles, 4-column tail
          (4360, 4100, 64)]       # 306 tiles on 256 CUs: several tiles per workgroup, statistics / bias pieces fetched at every tile start
BIG = (4360, 4100, 64)
PADDED_SHAPES = [(129, 264, 192), (257, 260, 192)]
GELU_SHAPES = [(129, 264, 192), (257, 260, 192)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib
    return _lib.load()


@pytest.fixture(params=sorted(KERNELS), ids=[KERNEL_IDS[k] for k in sorted(KERNELS)])
def sel(request):
    from hirest_amd import ops
    ops.gemm_select_kernel(request.param)
    try:
        yield request.param
    finally:
        ops.gemm_select_kernel(0)


def _stats_buffer(mean, rstd):
    """f32 [M rounded up to even, 2] = (mean, rstd): the header asks for a buffer readable up to an even row count."""
    M = mean.shape[0]
    st = torch.zeros((M + (M & 1), 2), dtype=torch.float32)
    st[:, 1] = 1.0
    st[:M, 0] = mean
    st[:M, 1] = rstd
    return st


def fold_exact(M, N, K):
    """a, w, bias of X.gemm_exact plus integer row means in [-4, 4], rstd in {0.5, 1, 2} and s = the integer row sums of w; `want` is the exact
    result in fp64 rounded to bf16 once.  Asserts that every intermediate is a half-integer below 2^23, i.e. an fp32 number."""
    d = X.gemm_exact(M, N, K)
    rng = np.random.default_rng([41, M, N, K])
    mean = torch.from_numpy(rng.integers(-4, 5, size=(M,)).astype(np.float32))
    rstd = torch.from_numpy(rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=(M,)))
    s = d["w"].float().sum(1)
    acc, s64, b64 = d["ref"].double(), s.double(), d["bias"].double()
    assert torch.equal(s64, d["w"].double().sum(1))                                  # the fp32 row sums are the integer sums
    c = -(mean.double() * rstd.double())
    scaled, shift = acc * rstd.double()[:, None], s64[None, :] * c[:, None]
    inner = shift + b64[None, :]
    want = scaled + inner + 0.0
    for t in (acc, scaled, shift, inner, want):
        assert torch.equal(t * 2, (t * 2).round()) and 2 * t.abs().max().item() < X.F32_EXACT
    want32 = want.float()
    assert torch.equal(want32.double(), want)
    assert X.bf16_ties(want32).any()                                                 # the rounding rule is exercised, not only exact values
    return {"a": d["a"], "w": d["w"], "bias": d["bias"], "s": s, "stats": _stats_buffer(mean, rstd), "want": want32.to(torch.bfloat16),
            "want_nobias": (scaled + shift + 0.0).float().to(torch.bfloat16)}


_CACHE = {}


def _data(M, N, K, dev):
    """The inputs and the expected bits of a shape on the device, computed once."""
    key = (M, N, K)
    if key not in _CACHE:
        _CACHE[key] = {k: v.to(dev) for k, v in fold_exact(M, N, K).items()}
    return _CACHE[key]


def _gemm(lib, expect, a, w, bias, out, ldo, M, N, K, epi, stats, s, flags=0):
    from hirest_amd import _lib, ops
    args = _lib.GemmArgs.make(a.data_ptr(), K, w.data_ptr(), K, None if bias is None else bias.data_ptr(), out.data_ptr(), ldo, M, N, K, epi,
                              None, 0, stats.data_ptr(), s.data_ptr(), int(flags))
    name = C.create_string_buffer(64)
    _lib.check(lib.hirest_gemm_dispatch_name(C.byref(args), name, 64), "hirest_gemm_dispatch_name")
    assert name.value.decode() == expect
    _lib.check(lib.hirest_gemm_bf16(C.byref(args), ops.stream_ptr()), "hirest_gemm_bf16")


def _sentinel(shape, dev):
    return torch.full(shape, SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))


def _run_exact(lib, dev, sel, M, N, K, pad_o=0, flags=0, bias=True):
    """One exact call into a sentinel-filled [M + GUARD_ROWS, N + pad_o] buffer: rows < M, columns < N hold the expected bits and every other
    element (pad columns, guard rows) its sentinel."""
    d = _data(M, N, K, dev)
    ldo = N + pad_o
    buf = _sentinel((M + GUARD_ROWS, ldo), dev)
    exp = buf.clone()
    exp[:M, :N] = d["want"] if bias else d["want_nobias"]
    _gemm(lib, KERNELS[sel] % EPI_FOLD, d["a"], d["w"], d["bias"] if bias else None, buf, ldo, M, N, K, EPI_FOLD, d["stats"], d["s"], flags)
    assert _same_bits(buf, exp), (sel, M, N, K, pad_o, flags, bias)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fold_exact_at_tile_edges(dev, lib, sel, M, N, K):
    _run_exact(lib, dev, sel, M, N, K)


@pytest.mark.parametrize("pad_o", [8, 4])
@pytest.mark.parametrize("M,N,K", PADDED_SHAPES)
def test_fold_untouched_memory(dev, lib, sel, M, N, K, pad_o):
    """ldo = N + 8 and ldo = N + 4 (rows then only 8-byte aligned): the pad columns and the three rows after M - 1 keep their sentinel."""
    _run_exact(lib, dev, sel, M, N, K, pad_o=pad_o)


def test_fold_without_bias_exact(dev, lib, sel):
    """bias = NULL means b' = 0 (the kernel must not add what it staged in the bias slot)."""
    _run_exact(lib, dev, sel, 129, 264, 192, bias=False)


def test_fold_reverse_walk_exact(dev, lib, sel):
    """HIREST_GEMM_REVERSE on more tiles than CUs: the backward walk gives the exact reference, hence the forward walk's bits."""
    from hirest_amd import _lib
    _run_exact(lib, dev, sel, *BIG, flags=_lib.GEMM_REVERSE)


@pytest.mark.parametrize("M,N,K", GELU_SHAPES)
def test_fold_gelu_per_element(dev, lib, sel, M, N, K):
    """HIREST_EPI_LNFOLD_GELU_BF16 with mean = 0, rstd = 1 on an exact pre-activation x = a w^T + b' (X.gemm_gelu) against x Phi(x) in fp64,
    per element: |out - g| <= ulp_bf16(g) / 2 + 4e-5 |g| + 2e-6 (X.gelu_bound); pad columns and guard rows untouched."""
    d = X.gemm_gelu(M, N, K)
    a, w, bias = d["a"].to(dev), d["w"].to(dev), d["bias"].to(dev)
    s = d["w"].float().sum(1).to(dev)
    stats = _stats_buffer(torch.zeros(M), torch.ones(M)).to(dev)
    ldo = N + 8
    out = _sentinel((M + GUARD_ROWS, ldo), dev)
    _gemm(lib, KERNELS[sel] % EPI_FOLD_GELU, a, w, bias, out, ldo, M, N, K, EPI_FOLD_GELU, stats, s)
    g = X.gelu_ref(d["x"])
    got = out[:M, :N].cpu().double()
    assert torch.isfinite(got).all()
    ratio = ((got - g).abs() / X.gelu_bound(g)).max().item()
    print(f"fold gelu epilogue {KERNELS[sel] % EPI_FOLD_GELU} {M}x{N}x{K}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert _same_bits(out[M:], _sentinel((GUARD_ROWS, ldo), dev)) and _same_bits(out[:M, N:], _sentinel((M, 8), dev))
