"""Inputs whose results are known without a tolerance, and the fp64 references that go with them, for tests/test_gpu_gemm_exact.py,
tests/test_gpu_attention_edges.py, tests/test_gpu_attention_x3_exact.py and tests/test_gpu_gemm_f32_exact.py.  tests/test_exact_inputs_host.py checks every precondition stated here on the CPU, so a wrong
generator cannot make a GPU test pass vacuously.  Not a test module.

"Exact inputs" for the bf16 GEMM: operands are small integers (or integers times a power of two), so every product and every
partial sum is an integer multiple of one power of two and smaller than 2^24 times it: fp32 accumulation is exact in ANY order, and
the result of every kernel, tile walk and split-K order is one known bit pattern."""
import math

import numpy as np
import torch

F32_EXACT = 2 ** 24          # integers of magnitude up to 2^24 are fp32 numbers

# (M, N, K) of tests/test_gpu_gemm_exact.py: tile-edge neighbours of the 128 and 256 tiles, one row, a deep K, and more 256 x 256 tiles
# (18 x 17 = 306) than the 256 CUs so the persistent kernels walk more than one tile per workgroup
GEMM_SHAPES = [(1, 4, 64), (63, 260, 448), (127, 124, 64), (128, 128, 64), (129, 132, 128), (255, 252, 192), (256, 256, 192),
               (257, 260, 192), (385, 644, 128), (257, 260, 6144), (4360, 4100, 64)]
GEMM_BIG = (4360, 4100, 64)
GEMM_STRIDED_SHAPES = [(129, 132, 128), (257, 260, 192)]
GEMM_GELU_SHAPES = [(129, 132, 128), (257, 260, 192)]
GEMM_LNSTATS_SHAPES = [(64, 256, 64), (129, 264, 192)]
# M = B * P of the patch-embed epilogue, per M above
PATCH_FRAMES = {1: 1, 63: 3, 127: 1, 128: 2, 129: 3, 255: 5, 256: 4, 257: 1, 385: 5, 4360: 8}
# split-operand cases: (M, N, original K); the GEMM's K argument is twice that
X3_SHAPES = [(131, 132, 64), (1, 4, 32), (2060, 2048, 32), (4360, 4100, 32), (300, 260, 512)]
X3_GELU_SHAPE = (257, 288, 64)
X3_FRAC = 2.0 ** -10


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _ints(rng, shape, lo, hi):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


_GEMM_CACHE = {}


def gemm_exact(M, N, K):
    """a [M, K], w [N, K] bf16 integers in [-3, 3]; bias [N], resid [M, N], pos [P + 1, N] fp32 integers in [-8, 8]; ref = a w^T (fp32,
    exact).  Every 16th row of a is all 3 and two of every 8 rows of w are non-negative, so some sums exceed 256 at every K: there bf16 keeps
    fewer bits than the integer has, and odd values are exact ties of the bf16 rounding."""
    key = (M, N, K)
    if key not in _GEMM_CACHE:
        if len(_GEMM_CACHE) >= 2:
            _GEMM_CACHE.pop(next(iter(_GEMM_CACHE)))
        rng = _rng(11, M, N, K)
        a, w = _ints(rng, (M, K), -3, 3), _ints(rng, (N, K), -3, 3)
        a[0::16] = 3.0
        w[0::8] = w[0::8].abs()
        w[1::8] = w[1::8].abs()
        P = M // PATCH_FRAMES.get(M, 1)
        bias, ref = _ints(rng, (N,), -8, 8), a @ w.t()
        # (in [256, 512) bf16 keeps even integers: 1 mod 4 is a tie that rounds down, 3 mod 4 one that rounds up; the one-row shape gets both)
        for col, residue in ((0, 1), (1, 3)):
            if 256 <= ref[0, col] < 500:
                bias[col] = (residue - ref[0, col]) % 4
        d = {"a": a.to(torch.bfloat16), "w": w.to(torch.bfloat16), "bias": bias, "resid": _ints(rng, (M, N), -8, 8),
             "pos": _ints(rng, (P + 1, N), -8, 8), "P": P, "ref": ref}
        _GEMM_CACHE[key] = d
    return _GEMM_CACHE[key]


def gemm_lnstats(M, N, K):
    """The same integers for the LN-statistics producer, with a milder structure (every 16th row of a and every 8th row of w non-negative; all-3 rows
    only at K <= 64): x = resid + a w^T + bias still passes 256, where bf16 rounds, but the sum of x^2 over a row stays below 2^24."""
    rng = _rng(14, M, N, K)
    a, w = _ints(rng, (M, K), -3, 3), _ints(rng, (N, K), -3, 3)
    a[0::16] = 3.0 if K <= 64 else a[0::16].abs()                  # (sums of about 330 at K = 64 and about 560 at K = 192)
    w[0::8] = w[0::8].abs()
    return {"a": a.to(torch.bfloat16), "w": w.to(torch.bfloat16), "bias": _ints(rng, (N,), -8, 8), "resid": _ints(rng, (M, N), -8, 8), "ref": a @ w.t()}


def bf16_ties(t):
    """Elements of the fp32 tensor t that lie exactly halfway between two bf16 numbers."""
    return (t.contiguous().view(torch.int32) & 0xFFFF) == 0x8000


def gelu_shift(K):
    """s with the pre-activation's standard deviation sqrt(4 K / 9) 2^-s nearest 3 (a, w uniform on {-1, 0, 1}: variance 2/3 each)."""
    return max(0, round(0.5 * math.log2(4.0 * K / 81.0)))


def gemm_gelu(M, N, K):
    """a in {-1, 0, 1}, w in {-1, 0, 1} * 2^-s (bf16), bias in multiples of 1/8 in [-2, 2]: x = a w^T + bias is exact in fp32."""
    rng = _rng(12, M, N, K)
    s = gelu_shift(K)
    a, w = _ints(rng, (M, K), -1, 1), _ints(rng, (N, K), -1, 1) * 2.0 ** -s
    bias = _ints(rng, (N,), -16, 16) / 8.0
    return {"a": a.to(torch.bfloat16), "w": w.to(torch.bfloat16), "bias": bias, "x": a @ w.t() + bias, "s": s}


def gelu_ref(x):
    """nn.GELU() (erf form) in fp64: x Phi(x)."""
    x = x.double()
    return x * 0.5 * torch.erfc(-x / math.sqrt(2.0))


def qgelu_ref(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def ulp_bf16(g):
    """Spacing of the bf16 numbers around g (fp64 tensor): 2^(floor(log2 |g|) - 7); 0 at 0."""
    m, e = torch.frexp(g.double().abs())              # |g| = m 2^e, m in [0.5, 1)
    return torch.where(g == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), e - 1 - 7))


def gelu_bound(g):
    """|out - g| allowed for a bf16 store of an fp32 GELU: half a bf16 ulp, plus twice the fp32 error csrc/common.h documents for gelu_erf
    (2e-5 relative, 1.1e-6 absolute).  Worst error / bound observed on the MI355X: GELU 0.963, QuickGELU 0.958."""
    return ulp_bf16(g) / 2 + 4e-5 * g.abs() + 2e-6


def split2_cpu(x):
    """[rows, D] fp32 -> [rows, 2 D] bf16 in the format ops.split2 documents: per 64 output columns, the hi parts of 32 consecutive input
    columns, then their lo parts (hi = bf16(x), lo = bf16(x - hi))."""
    rows, D = x.shape
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    out = torch.empty((rows, D // 32, 2, 32), dtype=torch.bfloat16)
    out[:, :, 0] = hi.reshape(rows, D // 32, 32)
    out[:, :, 1] = lo.reshape(rows, D // 32, 32)
    return out.reshape(rows, 2 * D)


def unsplit2_cpu(x2):
    """hi + lo of a split operand, in fp32."""
    rows, D2 = x2.shape
    return x2.reshape(rows, D2 // 64, 2, 32).float().sum(dim=2).reshape(rows, D2 // 2)


def gemm_x3(M, N, K, frac_in_a):
    """Split-operand case: one operand integer + integer * 2^-10 (both in [-3, 3]), the other integer: its lo part is 0, so the lo * lo
    product the kernel drops is 0 and hi-hi + hi-lo + lo-hi is the whole product.  a, w fp32 values; a2, w2 their split forms."""
    rng = _rng(13, M, N, K, int(frac_in_a))
    a, w = _ints(rng, (M, K), -3, 3), _ints(rng, (N, K), -3, 3)
    if frac_in_a:
        a = a + _ints(rng, (M, K), -3, 3) * X3_FRAC
    else:
        w = w + _ints(rng, (N, K), -3, 3) * X3_FRAC
    return {"a": a, "w": w, "a2": split2_cpu(a), "w2": split2_cpu(w), "bias": _ints(rng, (N,), -8, 8), "resid": _ints(rng, (M, N), -8, 8),
            "ref": (a.double() @ w.double().t()).float()}


def gemm_x3_gelu(M, N, K):
    """The GELU inputs as split operands (both lo parts 0)."""
    d = gemm_gelu(M, N, K)
    d["a2"], d["w2"] = split2_cpu(d["a"].float()), split2_cpu(d["w"].float())
    return d


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
ATTN_N = [1, 15, 16, 17, 64, 79, 80, 81, 96, 255, 256, 257, 271, 272]
ATTN_H = 2


def pack_qkv(q, k, v):
    """q, k, v [B, N, H, dh] -> the packed activation [B * N, 3 * H * dh] (columns: which, head, dh), bf16."""
    B, N, H, dh = q.shape
    return torch.stack([q, k, v], dim=2).reshape(B * N, 3 * H * dh).to(torch.bfloat16)


def unpack_qkv(qkv, B, N, H, dh):
    q, k, v = qkv.reshape(B, N, 3, H, dh).unbind(2)
    return q, k, v


def admitted(N, causal):
    """[N queries, N keys] bool: key j is visible to query i."""
    m = torch.ones((N, N), dtype=torch.bool)
    return m.tril() if causal else m


def attention_logits(qkv, B, N, H, dh):
    """Natural-unit logits scale * q . k in fp64, [B, H, N, N]."""
    q, k, _ = unpack_qkv(qkv.double(), B, N, H, dh)
    return torch.einsum("bihd,bjhd->bhij", q, k) * dh ** -0.5


def attention_ref(qkv, B, N, H, dh, causal):
    """softmax(scale q k^T [+ causal mask]) v in fp64, [B * N, H * dh]."""
    s = attention_logits(qkv, B, N, H, dh).masked_fill(~admitted(N, causal), float("-inf"))
    v = unpack_qkv(qkv.double(), B, N, H, dh)[2]
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, -1), v).reshape(B * N, H * dh)


def column_max_admitted(qkv, B, N, H, dh, causal):
    """max over the keys j visible to query i of |v[b, j, h, d]|, [B * N, H * dh] fp64: the scale of the per-element bound."""
    v = unpack_qkv(qkv.double(), B, N, H, dh)[2].abs()
    m = torch.cummax(v, dim=1).values if causal else v.amax(dim=1, keepdim=True).expand_as(v)
    return m.reshape(B * N, H * dh)


def _distinct_v(rng, shape):
    """Non-zero bf16 values with random sign, exponent in {-1, 0, 1} and a random 7-bit significand: two different (frame, head, key)
    rows agree in all dh columns with probability 2^-9dh."""
    bits = (rng.integers(0, 2, size=shape) << 15) | (rng.integers(126, 129, size=shape) << 7) | rng.integers(0, 128, size=shape)
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def attn_selector(B, N, H, dh, causal, seed):
    """Family 1.  k_j are random +-1 rows and q_i = 32 k_pi(i): the selected logit 32 sqrt(dh) exceeds every other by more than 64, so its p is
    exactly 1, every other p is below 2^-92 and vanishes against it in fp32: out[b, i, h] == v[b, pi(i), h] bit for bit.  pi is a random
    permutation per (frame, head), or a random pi(i) <= i when causal with pi(i) = i at i % 3 == 0 and pi(i) = 0 at i % 3 == 1."""
    rng = _rng(21, B, N, H, dh, int(causal), seed)
    k = torch.from_numpy(rng.integers(0, 2, size=(B, N, H, dh)).astype(np.float32) * 2 - 1)
    if causal:
        pi = rng.integers(0, np.arange(N)[None, None, :] + 1, size=(B, H, N))
        pi[:, :, 0::3] = np.arange(N)[0::3]
        pi[:, :, 1::3] = 0
    else:
        pi = np.stack([np.stack([rng.permutation(N) for _ in range(H)]) for _ in range(B)])
    pi = torch.from_numpy(pi.astype(np.int64))                                        # [B, H, N]
    idx = pi.permute(0, 2, 1)[..., None].expand(B, N, H, dh)                          # gather along the key axis
    q = 32.0 * torch.gather(k, 1, idx)
    v = _distinct_v(rng, (B, N, H, dh))
    want = torch.gather(v.view(torch.int16), 1, idx).view(torch.bfloat16).reshape(B * N, H * dh)
    return {"qkv": pack_qkv(q, k, v.float()), "pi": pi, "want": want}


def selector_gap(d, B, N, H, dh, causal):
    """Smallest (selected logit - largest other visible logit) over all rows, in natural units, from the fp64 logits."""
    s = attention_logits(d["qkv"], B, N, H, dh).masked_fill(~admitted(N, causal), float("-inf"))
    sel = torch.gather(s, 3, d["pi"][..., None])
    rest = s.scatter(3, d["pi"][..., None], float("-inf")).amax(-1, keepdim=True)
    return (sel - rest).min().item() if N > 1 else float("inf")


def attn_uniform(B, N, H, dh, causal, seed):
    """Family 2.  q = 0: every visible p is exactly 1.  V[j, d] = 1 if j % dh == d else 0, so out[i, d] = (visible keys j with j % dh == d) /
    (visible keys): one key too many or too few moves some column by at least 1 / (count + 1) >= 20 %."""
    rng = _rng(22, B, N, H, dh, int(causal), seed)
    k = torch.from_numpy(rng.standard_normal((B, N, H, dh)).astype(np.float32))
    q = torch.zeros((B, N, H, dh))
    v = ((torch.arange(N)[:, None] % dh) == torch.arange(dh)[None, :]).float()[None, :, None, :].expand(B, N, H, dh)
    adm = admitted(N, causal).double()
    keys = adm.sum(1)                                                                  # [N]
    ref = (adm @ v[0, :, 0].double()) / keys[:, None]                                  # [N, dh]
    ref = ref[None, :, None, :].expand(B, N, H, dh).reshape(B * N, H * dh)
    return {"qkv": pack_qkv(q, k, v), "ref": ref, "keys": keys.long()}


def uniform_bound(ref):
    """out = bf16(count * fl(1 / keys)): half a bf16 ulp of the quotient, plus 2^-19 relative and 2^-24 absolute for the two fp32 roundings
    before it (they can also move the value across a rounding midpoint).
    The first term was first written as 2^-9 |ref|.  That is half an ulp only for significands near 2: bf16 keeps 8 significant bits, so half an
    ulp is between 2^-9 |ref| and 2^-8 |ref| (1 / 15 = 1.0667 * 2^-4 rounds with an error of 1.87 * 2^-9 |ref| in every kernel and in
    torch's own bf16 cast).  The term is the rounding of the bf16 store itself; the kernels are right and the derivation was corrected.
    The slack terms are the original ones (2^-9 * 2^-10 = 2^-19).  Worst error / bound observed on the MI355X: 0.995 (against the first form
    of the bound: 1.98)."""
    return ulp_bf16(ref) / 2 + 2.0 ** -19 * ref.abs() + 2.0 ** -24


def attn_isolation(B, N, H, dh, causal, seed):
    """Family 3.  Within a frame every logit is about -200: q = -c s_b u and k = s_b (u + small) with u a +-1 vector per head, c = 200 /
    sqrt(dh) and s_b = +1 / -1 in even / odd frames.  A key borrowed from the neighbouring frame meets q with the other sign: logit +200,
    400 above the real ones, so it would take the whole softmax."""
    rng = _rng(23, B, N, H, dh, int(causal), seed)
    u = torch.from_numpy(rng.integers(0, 2, size=(1, 1, H, dh)).astype(np.float32) * 2 - 1)
    sgn = torch.tensor([1.0, -1.0]).repeat((B + 1) // 2)[:B].reshape(B, 1, 1, 1)
    small = torch.from_numpy(rng.standard_normal((B, N, H, dh)).astype(np.float32)) * 2.0 ** -4
    c = 200.0 / math.sqrt(dh)
    q = (-c * sgn * u).expand(B, N, H, dh)
    k = sgn * (u + small)
    v = torch.from_numpy(rng.standard_normal((B, N, H, dh)).astype(np.float32))
    return {"qkv": pack_qkv(q, k, v)}


def attn_random(B, N, H, dh, causal, qscale):
    """Family 4: the inputs of test_gpu_parity.py::test_attention, with V column 1 of every head scaled by 64 and column 2 by 1 / 64 (a
    bound relative to the tensor's maximum would be blind to the small column)."""
    from hirest_amd import synth
    D = H * dh
    x = synth.tensor(f"at.{N}.{dh}", (B * N, 3 * D), 1.0, 9).to(torch.bfloat16).float()
    x[:, :D] *= qscale
    vv = x[:, 2 * D:].reshape(B * N, H, dh)
    vv[:, :, 1] *= 64.0
    vv[:, :, 2] /= 64.0
    return {"qkv": x.to(torch.bfloat16)}


def attention_bound(colmax):
    """|out - ref| per element: three bf16 roundings of at most 2^-9 each relative to the column maximum over the visible keys (P, the
    fp32 normaliser's mismatch with the rounded P, the output) and a fourth 2^-9 for the fp32 score and exp2 error.  Worst error / bound
    observed on the MI355X: 0.605 on random inputs, 0.598 on the isolation inputs."""
    return 2 * 2.0 ** -8 * colmax


# Which launcher of csrc/attention.hip a call reaches: copied from the dispatch in hirest_attention_bf16_rows.
def attention_launcher(variant, B, N, dh, causal):
    """(launcher, DH, NT, FAST, causal[, variant]) — the template instantiation and the causal flag it runs with."""
    if variant >= 3 and 80 < N <= 272 and B >= 64:
        return ("launch3", dh, 17, (not causal) and N > 256, bool(causal), variant)
    nt = 5 if N <= 80 else 17
    return ("launch2" if variant >= 2 else "launch", dh, nt, None, bool(causal))


def attention_launchers_all():
    """Every instantiation the entry can reach, with both causal settings where the instantiation takes both (FAST is non-causal only)."""
    out = set()
    for dh in (64, 88):
        for nt in (5, 17):
            for c in (False, True):
                out.add(("launch", dh, nt, None, c))
                out.add(("launch2", dh, nt, None, c))
        for variant in (3, 4, 5, 6, 7):
            out.add(("launch3", dh, 17, True, False, variant))
            out.add(("launch3", dh, 17, False, False, variant))
            out.add(("launch3", dh, 17, False, True, variant))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# split-operand attention (csrc/attention_x3.hip): tests/test_gpu_attention_x3_exact.py
#   fp32 q [B, Tq, H, dh], k and v [B, Tk, H, dh]; head scale dh ** -0.5; both products from bf16 hi + lo parts of both operands
# ------------------------------------------------------------------------------------------------------------------------------
# (Tq, Tk) in query waves x key tiles: 1 x 1; 1 x 1 full; 2 x 1; 1 x 2; 2 x 3 (the first fetch at k0 + 64); 4 x 2; 5 x 4 (workgroups of
# 3 + 2 waves, or of 4 + 1); 10 x 2 (more than one nine-wave workgroup); 2 x 10
X3A_SHAPES = [(1, 1), (32, 32), (33, 31), (31, 33), (64, 65), (97, 64), (129, 97), (289, 33), (33, 289)]
X3A_DH = [4, 32, 36, 64, 68, 88, 96]          # 4: the dh - 4 clamp is 0; 36, 68: one group of four columns into the next DHP
X3A_B, X3A_H = [1, 3], [2, 3]
X3A_GAP = 110.0                               # exp(-110) = 2^-158.7 is below the smallest fp32 denormal (2^-149)
X3A_FRAC = 2.0 ** -10


def x3a_cases(dhs=None, passes=2):
    """A rotating subset of X3A_SHAPES x dhs x X3A_B x X3A_H: every shape `passes` times, with dh, B and H stepping at different rates so
    that every value of every axis occurs (asserted in tests/test_exact_inputs_host.py).  [(B, Tq, Tk, H, dh)]."""
    dhs = X3A_DH if dhs is None else dhs
    out = []
    for p in range(passes):
        for i, (Tq, Tk) in enumerate(X3A_SHAPES):
            n = p * len(X3A_SHAPES) + i
            out.append((X3A_B[n % 2], Tq, Tk, X3A_H[(n // 2) % 2], dhs[(n + 2 * p) % len(dhs)]))
    return out


def x3a_id(case):
    return "B{}-Tq{}-Tk{}-H{}-dh{}".format(*case)


def hi_lo(x):
    """The two bf16 parts the kernels form from an fp32 tensor, as fp32: hi = bf16(x), lo = bf16(x - hi)."""
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def _heads(t):
    return t.permute(0, 2, 1, 3)                  # [B, T, H, dh] <-> [B, H, T, dh]


def attention_x3_ref(q, k, v):
    """softmax(dh^-0.5 q k^T) v in fp64, [B, Tq, H, dh]."""
    q, k, v = (_heads(t.double()) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5
    return _heads(torch.softmax(s, -1) @ v)


def attention_x3_restated(q, k, v):
    """The same in fp64 from the bf16 hi + lo parts of q, k, p = exp(s - row max) and v, each product hi lo + lo hi + hi hi, normalised at
    the end (_whisper_enc_ref.attention_heads): what the operand format alone costs.  The yardstick of the random family."""
    import _whisper_enc_ref as W
    return _heads(W.attention_heads(*(_heads(t.double()) for t in (q, k, v)), True))


def attention_x3_logits(q, k):
    """Natural-unit logits in fp64, [B, H, Tq, Tk]."""
    return _heads(q.double()) @ _heads(k.double()).transpose(-1, -2) * q.shape[-1] ** -0.5


def attention_x3_emulated(q, k, v, drop=()):
    """The kernel's arithmetic in fp32 torch: 32-key tiles, the three score products added small terms first (k_hi q_lo, k_lo q_hi, k_hi
    q_hi), fp32 scale, running max with the exp(m_old - m_new) rescale, p split into hi + lo, v_hi p_lo + v_lo p_hi + v_hi p_hi, one
    division at the end.  The order of the additions inside a product is torch's, not the MFMA's.  `drop` names terms to leave out
    ("khql", "klqh", "vlph", ...): the host tests use it to show that a family notices a missing term."""
    B, Tq, H, dh = q.shape
    Tk = k.shape[1]
    scale = torch.tensor(dh ** -0.5, dtype=torch.float32)
    (qh, ql), (kh, kl), (vh, vl) = (tuple(_heads(p) for p in hi_lo(t.float())) for t in (q, k, v))
    term = lambda name, a, b: 0.0 if name in drop else a @ b
    o = torch.zeros((B, H, Tq, dh), dtype=torch.float32)
    mrun = torch.full((B, H, Tq, 1), -3.0e38, dtype=torch.float32)
    lrun = torch.zeros((B, H, Tq, 1), dtype=torch.float32)
    for k0 in range(0, Tk, 32):
        sl = slice(k0, min(k0 + 32, Tk))
        kht, klt = kh[:, :, sl].transpose(-1, -2), kl[:, :, sl].transpose(-1, -2)
        st = torch.zeros((B, H, Tq, sl.stop - k0), dtype=torch.float32)
        st = st + term("khql", ql, kht)
        st = st + term("klqh", qh, klt)
        st = (st + term("khqh", qh, kht)) * scale
        mnew = torch.maximum(mrun, st.amax(-1, keepdim=True))
        alpha = torch.exp(mrun - mnew)
        p = torch.exp(st - mnew)
        lrun = lrun * alpha + p.sum(-1, keepdim=True)
        mrun = mnew
        ph, pl = hi_lo(p)
        o = o * alpha
        o = o + term("vhpl", pl, vh[:, :, sl])
        o = o + term("vlph", ph, vl[:, :, sl])
        o = o + term("vhph", ph, vh[:, :, sl])
    return _heads(o * (1.0 / lrun))


def x3_column_max(v):
    """max over the keys of |v[b, j, h, d]|, [B, 1, H, dh] fp64: the scale of the per-element error of the random family."""
    return v.double().abs().amax(dim=1, keepdim=True)


def _balanced(rng, B, T, H, dh):
    """[B, T, H, dh] of +-1 with dh / 2 of each per vector, the T vectors of one (frame, head) pairwise distinct."""
    base = np.repeat(np.array([1.0, -1.0], dtype=np.float32), dh // 2)
    s = rng.permuted(np.broadcast_to(base, (B, T, H, dh)), axis=-1)
    for b in range(B):
        for h in range(H):
            while True:
                _, first = np.unique(s[b, :, h], axis=0, return_index=True)
                dup = np.setdiff1d(np.arange(T), first)
                if dup.size == 0:
                    break
                s[b, dup, h] = rng.permuted(np.broadcast_to(base, (dup.size, dh)), axis=-1)
    return torch.from_numpy(s)


def _x3_pi(rng, B, Tq, Tk, H):
    """pi [B, H, Tq] -> keys: every key when Tq >= Tk; always key Tk - 1 and one key of every 32-key tile; the rest random; shuffled."""
    tiles = (Tk + 31) // 32
    assert Tq >= min(Tk, tiles)
    pi = np.empty((B, H, Tq), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            if Tq >= Tk:
                must = rng.permutation(Tk)
            else:
                must = np.array([rng.integers(32 * t, min(32 * t + 32, Tk)) for t in range(tiles - 1)] + [Tk - 1], dtype=np.int64)
            row = np.concatenate([must, rng.integers(0, Tk, size=Tq - must.size)])
            pi[b, h] = rng.permutation(row)
    return torch.from_numpy(pi)


def _v16(rng, shape):
    """fp32 values with random sign, exponent in {-1, 0, 1} and a random 16-bit significand (the low 8 fraction bits are 0): v == hi + lo
    exactly, and lo != 0 for all but one value in 256, so an output is right only with both V parts."""
    bits = (rng.integers(0, 2, size=shape) << 31) | (rng.integers(126, 129, size=shape) << 23) | (rng.integers(0, 1 << 15, size=shape) << 8)
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32))


def _x3_selector(B, Tq, Tk, H, dh, seed, frac_in_k):
    assert dh >= 32 and dh % 2 == 0
    rng = _rng(31, B, Tq, Tk, H, dh, seed, int(frac_in_k))
    s = _balanced(rng, B, Tk, H, dh)
    pi = _x3_pi(rng, B, Tq, Tk, H)
    idx = pi.permute(0, 2, 1)[..., None].expand(B, Tq, H, dh)                         # gather along the key axis
    sel = torch.gather(s, 1, idx)
    if frac_in_k:
        q, k = sel, 1.0 + X3A_FRAC * s
    else:
        q, k = 1.0 + X3A_FRAC * sel, s
    # gap at c = 1 in fp64; the logits are linear in c
    c = 1.0 if Tk == 1 else 2.0 ** math.ceil(math.log2(X3A_GAP / x3_selector_gap({"q": q, "k": k, "pi": pi})))
    v = _v16(rng, (B, Tk, H, dh))
    return {"q": q * c, "k": k, "v": v, "pi": pi, "c": c, "s": s, "want": torch.gather(v, 1, idx)}


def x3_selector_klo(B, Tq, Tk, H, dh, seed=0):
    """k_j = u + 2^-10 s_j, q_i = c s_pi(i), with u all ones and s_j pairwise distinct balanced +-1 vectors (s . u = 0): bf16(k) = u and the
    lo part of k is 2^-10 s_j, both exactly, and q has no lo part, so the logits differ only through q_hi k_lo: c 2^-10 dh^-0.5 (s_pi(i) .
    s_j).  c is the smallest power of two that puts the selected logit at least X3A_GAP = 110 natural units above every other on every
    row (fp64): every other p and every rescale factor is 0 in fp32, the selected p and the normaliser are 1.  Every partial sum of either
    product is a multiple of c 2^-10 below 2^24 of it, hence exact in fp32 in any order; v has 16-bit significands (v == hi + lo).
    Guarantee: out[b, i, h] == v[b, pi(i), h] ("want") bit for bit."""
    return _x3_selector(B, Tq, Tk, H, dh, seed, True)


def x3_selector_qlo(B, Tq, Tk, H, dh, seed=0):
    """The mirror image: q_i = c (u + 2^-10 s_pi(i)), k_j = s_j.  bf16(q) = c u, the lo part of q is c 2^-10 s_pi(i), k has no lo part: the
    selection rides on q_lo k_hi alone.  Same guarantee."""
    return _x3_selector(B, Tq, Tk, H, dh, seed, False)


def x3_selector_gap(d):
    """Smallest (selected logit - largest other logit) over all rows, natural units, fp64."""
    lg = attention_x3_logits(d["q"], d["k"])
    top = torch.gather(lg, 3, d["pi"][..., None])
    rest = lg.scatter(3, d["pi"][..., None], float("-inf")).amax(-1, keepdim=True)
    return (top - rest).min().item() if lg.shape[-1] > 1 else float("inf")


def x3_uniform(B, Tq, Tk, H, dh, seed=0):
    """q = 0 (every p is exactly 1; k is random) and V[j, d] = 1 if j % dh == d else 0: out[i, d] = count_d / Tk with count_d the keys j <
    Tk with j % dh == d.  One key too many or too few moves a column by at least 1 / count of its value.
    bound = 2^-22 count_d / Tk: the sums are exact, the kernel rounds twice in fp32 (1 / Tk, then count_d times it), 2^-24 relative each,
    and the bound leaves a factor 2 on top of their sum."""
    rng = _rng(32, B, Tq, Tk, H, dh, seed)
    k = torch.from_numpy(rng.standard_normal((B, Tk, H, dh)).astype(np.float32))
    q = torch.zeros((B, Tq, H, dh))
    ind = ((torch.arange(Tk)[:, None] % dh) == torch.arange(dh)[None, :])
    ref = (ind.double().sum(0) / Tk)[None, None, None, :].expand(B, Tq, H, dh)
    return {"q": q, "k": k, "v": ind.float()[None, :, None, :].expand(B, Tk, H, dh).contiguous(), "ref": ref, "bound": ref * 2.0 ** -22}


def x3_isolation(B, Tq, Tk, H, dh, seed=0):
    """attn_isolation in fp32: q = -c s_b u and k = s_b (u + small) with u a +-1 vector per head, c = 200 / sqrt(dh) and s_b = +1 / -1 in
    even / odd frames.  Real logits are about -200; a key of the neighbouring frame meets q with the other sign (+200, 400 above), and
    the 3e38 the tests put after the keys would overflow the score."""
    rng = _rng(33, B, Tq, Tk, H, dh, seed)
    u = torch.from_numpy(rng.integers(0, 2, size=(1, 1, H, dh)).astype(np.float32) * 2 - 1)
    sgn = torch.tensor([1.0, -1.0]).repeat((B + 1) // 2)[:B].reshape(B, 1, 1, 1)
    small = torch.from_numpy(rng.standard_normal((B, Tk, H, dh)).astype(np.float32)) * 2.0 ** -4
    q = (-200.0 / math.sqrt(dh) * sgn * u).expand(B, Tq, H, dh).contiguous()
    v = torch.from_numpy(rng.standard_normal((B, Tk, H, dh)).astype(np.float32))
    return {"q": q, "k": sgn * (u + small), "v": v}


def x3_random(B, Tq, Tk, H, dh, qscale):
    """Standard normal q, k, v (fp32: every lo part is alive), q times qscale (1, 3, 6), V column 1 of every head times 64 and column 2
    times 1 / 64, so that an error bar relative to the tensor's maximum would be blind to column 2."""
    rng = _rng(34, B, Tq, Tk, H, dh, int(qscale))
    q, k, v = (torch.from_numpy(rng.standard_normal((B, T, H, dh)).astype(np.float32)) for T in (Tq, Tk, Tk))
    v[..., 1] *= 64.0
    v[..., 2] /= 64.0
    return {"q": q * qscale, "k": k, "v": v}


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 GEMM family (csrc/joint.hip): tests/test_gpu_gemm_f32_exact.py
# ------------------------------------------------------------------------------------------------------------------------------
F32_WMAX, F32_EPI_MAX = 15, 8          # |w| <= 15; |bias|, |resid|, |periodic| <= 8: the three addends together stay below 24


def f32_amax(K):
    """Largest |a| at which sum_k |a| |w| + 24 < 2^24 for every row pair: fp32 accumulation is then exact in any order."""
    return min(4095, (F32_EXACT - 1 - 3 * F32_EPI_MAX) // (F32_WMAX * K))


_F32_CACHE = {}


def gemm_f32_exact(M, N, K):
    """a [M, K] fp32 integers in [-amax, amax] (amax = f32_amax(K): 4095, i.e. 12 significant bits, up to K = 273), w [N, K] in [-15, 15],
    bias [N], resid [M, N], periodic [M + 3, N] in [-8, 8]; ref = a w^T (fp64).  Every 16th row of a is all +amax and two of every 8
    rows of w are non-negative, so the largest sums come near 15 K amax."""
    key = (M, N, K)
    if key not in _F32_CACHE:
        if len(_F32_CACHE) >= 2:
            _F32_CACHE.pop(next(iter(_F32_CACHE)))
        rng = _rng(31, M, N, K)
        amax = f32_amax(K)
        a, w = _ints(rng, (M, K), -amax, amax), _ints(rng, (N, K), -F32_WMAX, F32_WMAX)
        a[0::16] = float(amax)
        w[0::8] = w[0::8].abs()
        w[1::8] = w[1::8].abs()
        _F32_CACHE[key] = {"a": a, "w": w, "amax": amax, "bias": _ints(rng, (N,), -F32_EPI_MAX, F32_EPI_MAX),
                           "resid": _ints(rng, (M, N), -F32_EPI_MAX, F32_EPI_MAX), "periodic": _ints(rng, (M + 3, N), -F32_EPI_MAX, F32_EPI_MAX),
                           "ref": a.double() @ w.double().t()}
    return _F32_CACHE[key]


def f32_act_shift(K):
    """s with the pre-activation's standard deviation sqrt(4 K / 9) 2^-s nearest 1.5 (a, w uniform on {-1, 0, 1}): four standard deviations
    are the [-6, 6] in which erf, tanh and exp do all their work."""
    return max(0, round(math.log2(math.sqrt(4.0 * K / 9.0) / 1.5)))


def gemm_f32_act(M, N, K):
    """a in {-1, 0, 1}, w in {-1, 0, 1} * 2^-s, bias in multiples of 1/8 in [-2, 2]: x = a w^T + bias (fp64 here) is exact in fp32 in any
    order.  resid [M, N] and periodic [7, N] are integers in [-8, 8], added after the activation."""
    rng = _rng(32, M, N, K)
    s = f32_act_shift(K)
    a, w = _ints(rng, (M, K), -1, 1), _ints(rng, (N, K), -1, 1) * 2.0 ** -s
    bias = _ints(rng, (N,), -16, 16) / 8.0
    return {"a": a, "w": w, "bias": bias, "s": s, "x": a.double() @ w.double().t() + bias.double(),
            "resid": _ints(rng, (M, N), -F32_EPI_MAX, F32_EPI_MAX), "periodic": _ints(rng, (7, N), -F32_EPI_MAX, F32_EPI_MAX)}


def f32_act(x, act):
    """The epilogue's activation formula (csrc/joint.hip epilogue_apply4) in the precision of x: 1 gelu (erf), 2 tanh, 3 quick-gelu."""
    if act == 1:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    if act == 2:
        return torch.tanh(x)
    if act == 3:
        return x * (1.0 / (1.0 + torch.exp(-1.702 * x)))
    return x


def overlap_view(M, lda, K):
    """(buf, offset, gathered): a flat NaN-filled fp32 buffer whose floats offset .. offset + (M - 1) lda + K - 1 are integers in
    [-f32_amax(K), f32_amax(K)] — the overlapping view A[m, k] = buf[offset + m lda + k] (lda < K: rows share floats) — with at least 4 K
    NaN floats before and after it, and the [M, K] matrix the view means, gathered row by row.  offset % 4 == 0."""
    rng = _rng(33, M, lda, K)
    n = (M - 1) * lda + K
    offset = 4 * K
    buf = torch.full((offset + n + 4 * K,), float("nan"), dtype=torch.float32)
    amax = f32_amax(K)
    buf[offset:offset + n] = _ints(rng, (n,), -amax, amax)
    gathered = torch.stack([buf[offset + m * lda: offset + m * lda + K] for m in range(M)])
    return buf, offset, gathered


# Shapes of tests/test_gpu_gemm_f32_exact.py, per kernel: (dispatch name, entry point, select_kernel, ring_mode, [(M, N, K), ...]).
# tests/test_exact_inputs_host.py proves with hirest_gemm_f32_dispatch_name (cus = 256) that every shape reaches the kernel it is listed under.
F32_PLAIN = [
    ("tile64", "gemm", 1, 0, [(1, 4, 16), (63, 60, 48), (64, 64, 112), (65, 68, 128), (129, 132, 144), (66, 36, 240)]),
    ("tile64", "gemm", 0, 0, [(60, 8196, 48)]),
    ("tile64.split", "ws", 0, 0, [(257, 68, 1024), (300, 132, 1040), (321, 4, 1056)]),
    ("ring<4>", "gemm", 0, 2, [(257, 68, 64), (300, 132, 96), (321, 4, 160)]),
    ("skinny", "gemm", 0, 0, [(1, 4, 16), (31, 36, 48), (33, 28, 112), (256, 100, 176)]),
    ("skinny", "gemm", 2, 0, [(15, 20, 128)]),
    ("m16<1,1,8>", "gemm", 0, 0, [(1, 4, 32), (15, 20, 64), (16, 16, 1152)]),
    ("m16<1,1,3>", "gemm", 0, 0, [(17, 2052, 96), (32, 2048, 416)]),
    ("m16<1,2,6>", "gemm", 0, 0, [(16, 8196, 64), (9, 8200, 896)]),
    ("m16<2,2,2>", "gemm", 0, 0, [(17, 8212, 384)]),
    ("m16<2,1,6>", "gemm", 0, 0, [(33, 36, 32), (47, 52, 896), (256, 20, 64)]),
    ("m16<1,1,4>", "gemm", 0, 0, [(33, 20, 2048), (130, 36, 2080)]),
]
# the row-group streaming kernel: (name, entry point, (M, N, K)).  The chooser takes mt = 1 for every narrow N (the first four shapes: one
# row group with a ragged tile, 4, 11 and 21 row tiles); mt = 2 .. 5 need enough column tiles per stream, i.e. a wide N
F32_ROWS = [("rows<mt=1>", "rows_colmax", (33, 4, 768)), ("rows<mt=1>", "rows_colmax", (49, 20, 768)), ("rows<mt=1>", "rows_colmax", (161, 132, 768)),
            ("rows<mt=1>", "rows_colmax", (330, 36, 768)), ("rows<mt=2>", "gemm", (96, 8200, 768)), ("rows<mt=3>", "rows_colmax", (200, 2052, 768)),
            ("rows<mt=4>", "rows_colmax", (300, 8196, 768)), ("rows<mt=5>", "rows_colmax", (390, 2052, 768))]
F32_LAYOUT_SHAPE = (68, 132, 48)
F32_LAYOUTS = [("tile64", 0, 0), ("tile64<ak>", 1, 0), ("tile64<wk>", 0, 1), ("tile64<ak,wk>", 1, 1)]
# hirest_gemm_f32_ln: (name, (M, N, K), resid, ids)
F32_M16LN = [("m16ln<1,1,2>", (1, 4, 256), False, False), ("m16ln<2,1,2>", (15, 36, 512), False, False), ("m16ln<3,1,2>", (16, 2052, 768), False, False),
             ("m16ln<4,1,2>", (32, 20, 1024), False, False), ("m16ln<1,1,2>", (33, 36, 256), False, False), ("m16ln<3,1,2>", (256, 20, 768), True, False),
             ("m16ln<3,1,2>", (25, 36, 768), False, True)]
# the LM-head stream, N = 8196, K = 768: M = 1 and the upper edge of each of the nine instantiations
F32_STREAM_NK = (8196, 768)
F32_STREAM = [(1, "m16ln_stream<3,1,8,0>"), (2, "m16ln_stream<3,1,8,0>"), (5, "m16ln_stream<3,1,8,1>"), (7, "m16ln_stream<3,1,8,2>"),
              (10, "m16ln_stream<3,1,8,3>"), (12, "m16ln_stream<3,1,8,4>"), (16, "m16ln_stream<3,1,8,5>"), (20, "m16ln_stream<3,2,4,3>"),
              (26, "m16ln_stream<3,2,4,4>"), (32, "m16ln_stream<3,2,2,5>")]
# the row-group kernel's LayerNorm form: (hirest_gemm_f32_rows_ln_mode, (M, N, K), name); mode 0 runs the chooser (mt 1 .. 3)
F32_ROWS_LN = [(mode, s, "rows<mt=1,ln,mode=%d>" % mode) for mode in (1, 2) for s in ((33, 2052, 768), (49, 8196, 768), (257, 20, 768), (300, 36, 768))] + \
              [(0, (33, 2052, 768), "rows<mt=1,ln,mode=0>"), (0, (49, 8196, 768), "rows<mt=1,ln,mode=0>"), (0, (257, 20, 768), "rows<mt=1,ln,mode=0>"),
               (0, (300, 36, 768), "rows<mt=1,ln,mode=0>"), (0, (257, 2052, 768), "rows<mt=2,ln,mode=0>"), (0, (200, 8196, 768), "rows<mt=3,ln,mode=0>")]
# overlapping A: (lda, K, M, entry point, select_kernel, ring_mode, name), N = F32_OVERLAP_N
F32_OVERLAP_N = 36
F32_OVERLAP = [(80, 240, 1, "gemm", 0, 0, "skinny"), (80, 240, 31, "gemm", 0, 0, "skinny"), (80, 240, 33, "gemm", 0, 0, "skinny"),
               (80, 240, 66, "gemm", 1, 0, "tile64"), (80, 240, 257, "gemm", 0, 0, "tile64"),
               (128, 384, 1, "gemm", 0, 0, "m16<1,1,8>"), (128, 384, 31, "gemm", 0, 0, "m16<1,1,8>"), (128, 384, 33, "gemm", 0, 0, "m16<2,1,6>"),
               (128, 384, 66, "gemm", 0, 0, "m16<2,1,6>"), (128, 384, 257, "gemm", 0, 2, "ring<4>"),
               (128, 192, 1, "gemm", 0, 0, "m16<1,1,8>"), (128, 192, 33, "gemm", 0, 0, "m16<2,1,6>"), (128, 192, 66, "gemm", 2, 0, "skinny"),
               (128, 192, 257, "gemm", 1, 0, "tile64"), (128, 192, 257, "gemm", 0, 2, "ring<4>"),
               (1024, 1536, 257, "ws", 0, 0, "tile64.split")]
# activations 1, 2, 3: (name, entry point, select_kernel, (M, N, K))
F32_ACT = [("tile64", "gemm", 1, (65, 68, 128)), ("tile64.split", "ws", 0, (257, 68, 1024)), ("m16<2,1,6>", "gemm", 0, (47, 52, 896)),
           ("skinny", "gemm", 0, (33, 28, 112))]
# every epilogue-operand combination: one shape per kernel family, with rows past a tile boundary (indices into F32_PLAIN's rows)
F32_EPILOGUE = {"tile64": (129, 132, 144), "tile64.split": (300, 132, 1040), "ring<4>": (300, 132, 96), "skinny": (33, 28, 112),
                "m16<2,1,6>": (47, 52, 896)}

# Every instantiation the fp32 dispatch can reach, by the name hirest_gemm_f32_dispatch_name gives it.  (hirest_gemm_f32_layouts with a
# workspace also runs its three k-major instantiations in the split form: the same instantiations plus gemm_f32_quarters_kernel, both
# listed here.  rows<mt=1,ln,mode=1> and mode=2 are one instantiation under two launch geometries.)
F32_ALL_NAMES = sorted(
    ["tile64", "tile64.split", "tile64<ak>", "tile64<wk>", "tile64<ak,wk>", "ring<4>", "skinny"] +
    ["m16<1,1,8>", "m16<1,1,3>", "m16<1,2,6>", "m16<2,2,2>", "m16<2,1,6>", "m16<1,1,4>"] +
    ["m16ln<%d,1,2>" % nv for nv in (1, 2, 3, 4)] +
    ["m16ln_stream<3,1,8,%d>" % d1 for d1 in range(6)] + ["m16ln_stream<3,2,4,3>", "m16ln_stream<3,2,4,4>", "m16ln_stream<3,2,2,5>"] +
    ["rows<mt=%d>" % mt for mt in (1, 2, 3, 4, 5)] + ["rows<mt=%d,ln,mode=0>" % mt for mt in (1, 2, 3)] +
    ["rows<mt=1,ln,mode=1>", "rows<mt=1,ln,mode=2>"])


def f32_dispatch_cases():
    """Every call tests/test_gpu_gemm_f32_exact.py makes, as (expected name, entry point, M, N, K, query fields)."""
    out = []
    for name, entry, sel, ring, shapes in F32_PLAIN:
        out += [(name, entry, M, N, K, dict(select_kernel=sel, ring_mode=ring, has_workspace=entry == "ws")) for M, N, K in shapes]
    out += [(name, entry, M, N, K, {}) for name, entry, (M, N, K) in F32_ROWS]
    out += [(name, "layouts", *F32_LAYOUT_SHAPE, dict(a_kmajor=ak, w_kmajor=wk)) for name, ak, wk in F32_LAYOUTS]
    out += [(name, "ln", M, N, K, dict(has_resid=resid, has_ids=ids, has_ln_out=True)) for name, (M, N, K), resid, ids in F32_M16LN]
    for M, name in F32_STREAM:
        out += [(name, "ln", M, *F32_STREAM_NK, {}), (name, "ln_colmax", M, *F32_STREAM_NK, {})]
    out += [(name, "ln", M, N, K, dict(rows_ln_mode=mode, has_ln_out=True)) for mode, (M, N, K), name in F32_ROWS_LN]
    out += [(name, entry, M, F32_OVERLAP_N, K, dict(select_kernel=sel, ring_mode=ring, has_workspace=entry == "ws"))
            for _, K, M, entry, sel, ring, name in F32_OVERLAP]
    for name, entry, sel, (M, N, K) in F32_ACT:
        out.append((name, entry, M, N, K, dict(select_kernel=sel, has_workspace=entry == "ws", has_resid=True, has_periodic=True)))
    return out
