"""tests/_train_ref.py checked on the CPU, so that tests/test_gpu_train_block.py compares the device with a reference that has been
compared with torch: the block in eval mode against F.scaled_dot_product_attention / F.layer_norm / F.gelu, its autograd against
numerical differences with dropout on, the conditions of the exact-score builder at every shape of the grid, and the three mask sites."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _train_ref as T


@pytest.fixture(scope="module", params=list(T.CASES))
def case(request):
    shape = T.CASES[request.param]
    return (shape,) + T.exact_score_inputs(*shape, T.CASE_SEED[request.param])


def test_builder_conditions(case):
    """exact_score_inputs asserts them itself; here once more on what it returned, with the selection rows counted."""
    (B, Tn, H, W, mlp), params, x, dout = case
    T.check_conditions(params, x, B, Tn, H)
    assert params["wqkv"].shape == (3 * W, W) and params["w1"].shape == (mlp, W) and params["w2"].shape == (W, mlp)
    assert x.shape == dout.shape == (B * Tn, W) and all(t.dtype is torch.float32 for t in list(params.values()) + [x, dout])
    nz = (params["wqkv"][:2 * W] != 0).sum(1)
    assert int((nz == 1).sum()) > 0 and int((nz == 2).sum()) > 0
    assert params["wqkv"][2 * W:].abs().max().item() < 0.2 and params["wqkv"][2 * W:].std().item() > 0.02        # the value rows are ordinary data


def test_eval_mode_equals_torch(case):
    """drop = 0 in fp64 against torch's own attention, LayerNorm and GELU within 1e-12: the uniform -10000 drops out of the softmax,
    and the scores are exact, so the fp32 rounding of S changes nothing."""
    (B, Tn, H, W, mlp), params, x, _ = case
    got = T.block_ref(params, x, B, Tn, H, 0.0, T.SEEDS, torch.float64)
    p = {n: t.double() for n, t in params.items()}
    x = x.double()
    qkv = F.linear(x, p["wqkv"], p["bqkv"])
    heads_of = lambda t: t.reshape(B, Tn, H, 64).transpose(1, 2)
    q, k, v = (heads_of(qkv[:, i * W:(i + 1) * W]) for i in range(3))
    cx = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * Tn, W)
    a_pre = x + F.linear(cx, p["wo"], p["bo"])
    aa = F.layer_norm(a_pre, (W,), p["ln1_g"], p["ln1_b"], T.LN_EPS)
    hpre = F.linear(aa, p["w1"], p["b1"])
    hh = F.gelu(hpre)
    x_pre = aa + F.linear(hh, p["w2"], p["b2"])
    out = F.layer_norm(x_pre, (W,), p["ln2_g"], p["ln2_b"], T.LN_EPS)
    want = dict(qkv=qkv, cx=cx, a_pre=a_pre, aa=aa, hpre=hpre, hh=hh, x_pre=x_pre, out=out,
                P=torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1))
    assert set(want) == set(T.ACTS) == set(got)
    for name in T.ACTS:
        assert got[name].shape == want[name].shape, name
        assert (got[name] - want[name]).abs().max().item() <= 1e-12, name


def test_gradcheck_with_dropout_on():
    """torch.autograd.gradcheck on block_ref at the smallest shape of the grid with drop = 0.5 (masks are constants), and at
    (1, 3, 1, 64, 16) with the fp32 rounding of the scores off: a numerical difference of 1e-6 cannot see through a rounding to
    multiples of 2^-10, and at T = 1 the softmax is constant, so only the second one exercises the softmax's gradient."""
    for (B, Tn, H, W, mlp), rounded in ((T.CASES["one"], True), ((1, 3, 1, 64, 16), False)):
        params, x, _ = T.exact_score_inputs(B, Tn, H, W, mlp, 7)
        masks = T.block_masks(B, Tn, H, W, 0.5, T.SEEDS)
        assert all(0 < int((m == 0).sum()) < m.numel() for m in masks[1:])
        leaves = [x.double().requires_grad_(True)] + [params[n].double().requires_grad_(True) for n in T.PARAMS]

        def f(x, *ps):
            a = T.block_ref(dict(zip(T.PARAMS, ps)), x, B, Tn, H, 0.5, T.SEEDS, torch.float64, masks=masks, round_scores=rounded)
            return a["out"], a["hh"], a["cx"]
        assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-4, fast_mode=True)


def test_bf16_operand_yardstick():
    """bf16_operands rounds operands only: with operands that are bf16 numbers already (x and the selection rows) the product is
    the exact one, with Gaussian weights it moves by about 2^-9 of the summed magnitudes; dW is the unrounded dY^T X."""
    B, Tn, H, W, mlp = T.CASES["x3"]
    params, x, dout = T.exact_score_inputs(B, Tn, H, W, mlp, T.CASE_SEED["x3"])
    a64, dx64, g64 = T.block_ref_grads(params, x, dout, B, Tn, H, 0.1, T.SEEDS, torch.float64)
    abf, dxbf, gbf = T.block_ref_grads(params, x, dout, B, Tn, H, 0.1, T.SEEDS, torch.float64, bf16_operands=True)
    assert torch.equal(a64["qkv"][:, :2 * W], abf["qkv"][:, :2 * W]) and torch.equal(a64["P"], abf["P"])
    for name in ("cx", "a_pre", "aa", "hpre", "hh", "x_pre", "out"):
        rel = (abf[name] - a64[name]).abs().max().item() / a64[name].abs().max().item()
        assert 2.0 ** -14 < rel < 2.0 ** -6, (name, rel)
    assert torch.equal(g64["g_ln2_b"], gbf["g_ln2_b"])                           # column sums of dout: no product in front of them
    rel = (dxbf - dx64).abs().max().item() / dx64.abs().max().item()
    assert 2.0 ** -14 < rel < 2.0 ** -6, rel


def test_mask_sites(case):
    """The three masks of a case are pairwise different and each drops a fraction within 5 sigma of p.  (At case one the attention
    mask has a single element: 5 sigma is more than 1 there, so the fraction says nothing about it, and a comparison of fewer than
    64 elements is skipped; the residual masks of that case have 64 elements each.)"""
    (B, Tn, H, W, mlp), *_ = case
    assert len(set(T.SEEDS)) == 3
    for p in (0.1, 0.5):
        masks = T.block_masks(B, Tn, H, W, p, T.SEEDS)
        pf = float(np.float32(p))
        for m in masks:
            assert set(m.unique().tolist()) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
            frac = (m == 0).double().mean().item()
            assert abs(frac - pf) <= 5 * np.sqrt(pf * (1 - pf) / m.numel()), (p, frac)
        flat = [m.flatten() for m in masks]
        for i in range(3):
            for j in range(i + 1, 3):
                n = min(flat[i].numel(), flat[j].numel())
                if n >= 64:                                                       # (2^-64 that two different streams agree on 64 elements at p = 0.5)
                    assert not torch.equal(flat[i][:n], flat[j][:n]), (p, i, j)
    ones = T.block_masks(B, Tn, H, W, 0.0, T.SEEDS)
    assert all(bool((m == 1).all()) for m in ones)
