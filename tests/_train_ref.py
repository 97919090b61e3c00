"""One post-LN encoder block in train mode (include/hirest_hip.h: hirest_train_block) restated with plain torch ops on the CPU, for
tests/test_gpu_train_block.py; tests/test_train_block_ref_host.py checks the restatement itself without a GPU.

    qkv = x Wqkv^T + b (rows query | key | value, heads of 64);  S = fl32(fl32(q.k dh^-0.5) + (-10000));  P = softmax(S)
    cx = (P keep_attn) v;  a_pre = x + keep_ao (cx Wo^T + bo);  aa = LN1(a_pre);  hpre = aa W1^T + b1;  hh = gelu_erf(hpre)
    x_pre = aa + keep_out (hh W2^T + b2);  out = LN2(x_pre)

The keep factors are those of hirest_dropout_add_f32 (keep_scale below: 0 or fl32(1 / (1 - p)), counter = the element's flat index),
used as constants in whatever dtype the block runs in.  In float64 the whole block is differentiable by autograd (the fp32 rounding of
the scores is straight-through: the value is rounded, the gradient is the exact one).
"""
import numpy as np
import torch

PARAMS = ("wqkv", "bqkv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2", "ln2_g", "ln2_b")
ACTS = ("qkv", "P", "cx", "a_pre", "aa", "hpre", "hh", "x_pre", "out")
GRADS = tuple("g_" + n for n in PARAMS)
LN_EPS = float(np.float32(1e-12))
ADD_CONST = -10000.0


# ---- the dropout keep mask, restated from train.hip's keep_scale ---------------------------------------------------------------
def keep_scale(seed, idx, p):
    """fp32 factor of element `idx` (uint64 array): 0 where dropped, fl(1 / (1 - p)) where kept, 1 everywhere at p = 0."""
    idx = np.asarray(idx, dtype=np.uint64)
    if p <= 0:
        return np.ones(idx.shape, np.float32)
    with np.errstate(over="ignore"):
        z = idx + np.uint64((int(seed) & 0xFFFFFFFF) << 32) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    pf = np.float32(p)
    return np.where(u < pf, np.float32(0), np.float32(1) / (np.float32(1) - pf)).astype(np.float32)


# ---- the row bar of the kernel tests (tests/test_gpu_train_kernels.py, tests/test_gpu_train_block.py) ---------------------------------
def _within(err, bar, what, at=None):
    """err, bar: tensors of the same shape; prints the worst err / bar so that a run shows the margin (`at`: the input values,
    reported at the worst element)."""
    err, bar = err.double(), bar.double()
    r = (err / bar.clamp_min(1e-300)).flatten()
    i = int(r.argmax()) if r.numel() else 0
    ratio = r[i].item() if r.numel() else 0.0
    where = f" at input {at.flatten()[i].item():.6g}" if at is not None and r.numel() else ""
    print(f"{what}: worst err/bar {ratio:.3g}{where}")
    assert ratio <= 1.0 and not torch.isnan(err).any(), f"{what}: err/bar {ratio:.3g}{where}"


def _rows_close(got, ref, tol, what, floor=1e-3):
    """|got - ref| <= tol * (row scale), row = last dimension, scale = max |ref| over the row (at least floor * the tensor's
    max, so that a row which is exactly zero in both is compared against the tensor's scale)."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(-1, keepdim=True).clamp_min(floor * ref.abs().max().item() + 1e-300)
    _within((got - ref).abs(), tol * scale.expand_as(ref), what)


def block_masks(B, T, heads, width, drop, seeds):
    """The three keep-factor tensors of a block (fp32): attention probabilities [B, H, T, T] at index ((b H + h) T + i) T + j with
    seeds[0], attention.output [R, W] at r W + c with seeds[1], output [R, W] with seeds[2]."""
    R = B * T
    flat = lambda seed, n: torch.from_numpy(keep_scale(seed, np.arange(n, dtype=np.uint64), drop))
    return (flat(seeds[0], B * heads * T * T).view(B, heads, T, T), flat(seeds[1], R * width).view(R, width),
            flat(seeds[2], R * width).view(R, width))


def _bf16(t):
    return t.detach().to(torch.bfloat16).to(t.dtype)


class _LinearBf16(torch.autograd.Function):
    """y = x W^T + b with the operands of the forward product and of the dX product rounded to bf16 (the sums stay in the
    tensors' own precision); dW = dY^T X and db on the unrounded tensors, as precision 1 of the block keeps them in fp32."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _bf16(x) @ _bf16(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return _bf16(dy) @ _bf16(w), dy.t() @ x, dy.sum(0)


def _linear(x, w, b, bf16_operands):
    return _LinearBf16.apply(x, w, b) if bf16_operands else x @ w.t() + b


def layernorm(x, g, b):
    """biased variance, eps inside the root"""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + LN_EPS) * g + b


def gelu_erf(x):
    return 0.5 * x * torch.special.erfc(-x / np.sqrt(2.0))


def attention(qkv, B, T, heads, keep, add_const=ADD_CONST, round_scores=True):
    """qkv [B T, 3 H 64] -> (S, P, cx): S [B, H, T, T] = fl32(fl32(q.k dh^-0.5) + add_const) (rounded straight-through; an fp32 qkv
    is rounded by its own arithmetic), P = softmax(S), cx [B T, H 64] = (P keep) v."""
    W = qkv.shape[1] // 3
    dh = W // heads
    scale = float(np.float32(dh ** -0.5))
    heads_of = lambda t: t.reshape(B, T, heads, dh).permute(0, 2, 1, 3)
    q, k, v = heads_of(qkv[:, :W]), heads_of(qkv[:, W:2 * W]), heads_of(qkv[:, 2 * W:])
    s = q @ k.transpose(-1, -2) * scale
    S = s + add_const
    if round_scores and S.dtype is not torch.float32:
        S = S + ((s.detach().float() + np.float32(add_const)).to(S.dtype) - S.detach())
    P = torch.softmax(S, -1)
    cx = ((P * keep.to(P.dtype)) @ v).permute(0, 2, 1, 3).reshape(B * T, W)
    return S, P, cx


def block_ref(params, x, B, T, heads, drop, seeds, dtype, bf16_operands=False, masks=None, round_scores=True):
    """The block's forward in `dtype` on the CPU.  params: the twelve tensors of PARAMS by name; seeds = (seed_attn, seed_ao,
    seed_out).  Returns {name: tensor} for every activation the device keeps (ACTS).  bf16_operands: the "bf16 GEMM" yardstick of
    precision 1 — the operands of the four forward products (and of the four dX products of the backward) rounded to bf16.
    masks: block_masks(...) computed by the caller (they are constants; a gradcheck evaluates the block thousands of times)."""
    p = {n: params[n].to(dtype) for n in PARAMS}
    x = x.to(dtype)
    W = x.shape[1]
    keep_attn, keep_ao, keep_out = masks if masks is not None else block_masks(B, T, heads, W, drop, seeds)
    qkv = _linear(x, p["wqkv"], p["bqkv"], bf16_operands)
    _, P, cx = attention(qkv, B, T, heads, keep_attn, ADD_CONST, round_scores)
    a_pre = x + keep_ao.to(dtype) * _linear(cx, p["wo"], p["bo"], bf16_operands)
    aa = layernorm(a_pre, p["ln1_g"], p["ln1_b"])
    hpre = _linear(aa, p["w1"], p["b1"], bf16_operands)
    hh = gelu_erf(hpre)
    x_pre = aa + keep_out.to(dtype) * _linear(hh, p["w2"], p["b2"], bf16_operands)
    out = layernorm(x_pre, p["ln2_g"], p["ln2_b"])
    return dict(qkv=qkv, P=P, cx=cx, a_pre=a_pre, aa=aa, hpre=hpre, hh=hh, x_pre=x_pre, out=out)


def block_ref_grads(params, x, dout, B, T, heads, drop, seeds, dtype, bf16_operands=False, masks=None):
    """One backward from `dout`.  Returns (activations, dx, {g_wqkv, g_bqkv, g_wo, g_bo, g_ln1_g, g_ln1_b, g_w1, g_b1, g_w2, g_b2,
    g_ln2_g, g_ln2_b}), all detached, in `dtype`."""
    leaves = {n: params[n].detach().to(dtype).clone().requires_grad_(True) for n in PARAMS}
    x = x.detach().to(dtype).clone().requires_grad_(True)
    acts = block_ref(leaves, x, B, T, heads, drop, seeds, dtype, bf16_operands, masks)
    acts["out"].backward(dout.to(dtype))
    return {n: t.detach() for n, t in acts.items()}, x.grad, {"g_" + n: leaves[n].grad for n in PARAMS}


def sixteen(grads, width):
    """The sixteen parameter gradients of the model's block (query, key and value are separate Linears there): the twelve tensors
    of block_ref_grads / hirest_train_block_grads with g_wqkv and g_bqkv cut into their thirds."""
    out = {}
    for n in GRADS:
        if n in ("g_wqkv", "g_bqkv"):
            for k, part in enumerate("qkv"):
                out[n[:3] + part] = grads[n][k * width:(k + 1) * width]
        else:
            out[n] = grads[n]
    return out


# ---- the seeded problem -------------------------------------------------------------------------------------------------------------
def _randn(g, shape, std=1.0, mean=0.0):
    return torch.randn(shape, generator=g, dtype=torch.float64).mul_(std).add_(mean).float()


def exact_score_inputs(B, T, heads, width, mlp, seed):
    """A block problem whose attention scores are exact: (params, x, dout), fp32 tensors.

    The block adds -10000 to every score, and ulp(10000) = 2^-10 in fp32: two evaluations whose scores differ by 1e-6 round
    about 0.1 % of them to different multiples of 2^-10, which moves P by 2^-10 relative.  Here every evaluation has the same scores:
      * x: multiples of 1/4 of magnitude < 32 (at most 8 significant bits: the bf16x3 split leaves a zero low half);
      * query and key rows of Wqkv: signed selection rows, one or two non-zeros from {+-1, +-1/2}; their biases multiples of 1/8;
      * so q and k are multiples of 1/8 below 2^6, q.k a sum of 64 multiples of 2^-6 below 2^18: exact in fp32 in any order;
        dh = 64, scale = 1/8 exact: every score is a multiple of 2^-9, and fl32(s - 10000) = s - 10000.
    Everything else is seeded Gaussian data at the scales of synth.joint_state_dict: the value rows, Wo, W1, W2 (0.03), biases
    (0.02), LayerNorm gamma (1 +- 0.1) and beta (0.05); dout ~ N(0, 1).  The conditions are asserted (check_conditions)."""
    assert width == heads * 64, "heads of 64"
    g = torch.Generator().manual_seed(seed)
    R = B * T
    x = torch.round(_randn(g, (R, width)) * 4).clamp_(-127, 127) / 4
    wqkv = _randn(g, (3 * width, width), 0.03)
    sel = torch.zeros((2 * width, width))
    rows = torch.arange(2 * width)
    coef = torch.tensor([1.0, -1.0, 0.5, -0.5])
    c1 = torch.randint(0, width, (2 * width,), generator=g)
    c2 = (c1 + torch.randint(1, width, (2 * width,), generator=g)) % width          # a second column, never the first
    sel[rows, c1] = coef[torch.randint(0, 4, (2 * width,), generator=g)]
    two = torch.randint(0, 2, (2 * width,), generator=g).bool()
    sel[rows[two], c2[two]] = coef[torch.randint(0, 4, (2 * width,), generator=g)][two]
    wqkv[:2 * width] = sel
    bqkv = _randn(g, (3 * width,), 0.02)
    bqkv[:2 * width] = torch.randint(-2, 3, (2 * width,), generator=g).float() / 8
    params = dict(wqkv=wqkv, bqkv=bqkv, wo=_randn(g, (width, width), 0.03), bo=_randn(g, (width,), 0.02),
                  ln1_g=_randn(g, (width,), 0.1, 1.0), ln1_b=_randn(g, (width,), 0.05),
                  w1=_randn(g, (mlp, width), 0.03), b1=_randn(g, (mlp,), 0.02), w2=_randn(g, (width, mlp), 0.03), b2=_randn(g, (width,), 0.02),
                  ln2_g=_randn(g, (width,), 0.1, 1.0), ln2_b=_randn(g, (width,), 0.05))
    dout = _randn(g, (R, width))
    check_conditions(params, x, B, T, heads)
    return params, x, dout


def check_conditions(params, x, B, T, heads):
    """What exact_score_inputs promises (conditions, not measurements).  T = 1 has one score per row: its softmax is the constant 1,
    so the two conditions on the shape of a row (range >= 1, not one-hot) are asked of T > 1 only."""
    W = x.shape[1]
    assert torch.equal(x, x.to(torch.bfloat16).float()) and torch.equal(x * 4, torch.round(x * 4)), "x: multiples of 1/4 with 8 significant bits"
    wqk, bqk = params["wqkv"][:2 * W], params["bqkv"][:2 * W]
    nz = (wqk != 0).sum(1)
    assert bool(((nz == 1) | (nz == 2)).all()) and bool(torch.isin(wqk[wqk != 0].abs(), torch.tensor([1.0, 0.5])).all()), "selection rows"
    assert torch.equal(bqk * 8, torch.round(bqk * 8)), "q / k biases: multiples of 1/8"
    qk32 = x @ wqk.t() + bqk
    qk64 = x.double() @ wqk.double().t() + bqk.double()
    assert torch.equal(qk32.double(), qk64), "q and k in fp32 equal their fp64 values bit for bit"
    assert torch.equal(qk64 * 8, torch.round(qk64 * 8)) and qk64.abs().max().item() < 64
    heads_of = lambda t: t.reshape(B, T, heads, 64).permute(0, 2, 1, 3)
    s = heads_of(qk64[:, :W]) @ heads_of(qk64[:, W:]).transpose(-1, -2) * 0.125
    assert torch.equal(s * 512, torch.round(s * 512))
    assert torch.equal((s.float() + np.float32(ADD_CONST)).double(), s + ADD_CONST), "fl32(s - 10000) == s - 10000 for every score"
    if T > 1:
        assert (s.amax(-1) - s.amin(-1)).min().item() >= 1.0, "a softmax row is flat"
        assert torch.softmax(s, -1).float().amax(-1).max().item() < 1.0, "a softmax row is one-hot to fp32"
    g1, g2 = params["ln1_g"], params["ln2_g"]
    assert not bool((g1 == 1).any()) and not bool((g2 == 1).any())


# the grid of tests/test_gpu_train_block.py: (B, T, heads, width, mlp) and the precisions each case runs in
CASES = {"one": (1, 1, 1, 64, 16), "odd": (2, 65, 3, 192, 80), "x3": (3, 33, 2, 128, 96), "split": (1, 257, 1, 64, 1024)}
PRECISIONS = {"one": (0,), "odd": (0,), "x3": (0, 1), "split": (0, 1)}
CASE_SEED = {"one": 101, "odd": 102, "x3": 103, "split": 104}
SEEDS = (0x51A7, 0x51A8, 0xFFFFFFFF)          # seed_attn, seed_ao, seed_out (the last one: the top of the 32-bit range)
