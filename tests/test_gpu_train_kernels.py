"""The training-step entry points of csrc/train.hip, one at a time, against float64 torch on the CPU (autograd where there is a
backward), at the shapes where kernels go wrong: tails of every tile, unroll and wave, Tq != Tk, zero variance, saturated
activations, all-masked rows.  Each test calls its entry point through _lib.load() the way train._K does.

Bars (every one derived from the fp32 arithmetic of the operation, U = 2^-24 the fp32 unit roundoff; see each docstring):
  * integer, mask and copy work: exact;
  * elementwise kernels: a few roundings of the operands' magnitude (a few ulp);
  * reductions of up to a few thousand terms: about 1e-5 of the row's scale, or the classic n * U * sum|terms| bound of an n-term
    fp32 sum where the kernel's summation depth is known.
The dropout keep mask is restated in numpy (keep_scale of tests/_train_ref.py, the splitmix64 of (seed, index) of train.hip) and matched exactly.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _train_ref import _rows_close, _within, keep_scale          # shared with tests/test_gpu_train_block.py

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # fp32 unit roundoff
FMAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from hirest_amd import _lib
    return _lib.load()


def _s():
    from hirest_amd import ops
    return ops.stream_ptr()


def _p(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * offset


def _rand(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).mul_(std).add_(mean).float()


def _randint(lo, hi, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32)


def _dev(dev, *ts):
    """Device copies that stay referenced until the caller's launch: a temporary's block would go back to the caching allocator
    at once, and the next copy in the same argument list could land in it before the kernel runs."""
    return [None if t is None else t.to(dev) for t in ts]


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def test_keep_scale_restatement_is_splitmix64():
    """The restatement itself, against a plain-integer splitmix64 (no numpy wrap-around) at a few indices."""
    def ref(seed, i, p):
        m = (1 << 64) - 1
        z = (i + (seed << 32) + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return (z >> 40) / 16777216.0 >= float(np.float32(p))
    idx = [0, 1, 2, 255, 256, 1 << 32, (1 << 40) + 12345, (1 << 63) + 7]
    for seed in (0, 5, 0xFFFFFFFF):
        for p in (0.1, 0.5, 0.9):
            got = keep_scale(seed, np.array(idx, dtype=np.uint64), p) != 0
            assert got.tolist() == [ref(seed, i, p) for i in idx]


# ---- elementwise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9])
@pytest.mark.parametrize("with_resid", [False, True], ids=["plain", "resid"])
def test_dropout_add_keep_mask(dev, lib, p, with_resid):
    """y = resid + x * keep(seed, i) / (1 - p).  The keep mask must equal the restatement EXACTLY (dropped elements are exactly
    resid, or 0).  Kept values: fl(1 - p), fl(1 / that) and the product / fused add are at most 4 roundings of the operands'
    magnitude: |y - (resid + x / (1 - p))| <= 4 U (|x| / (1 - p) + |resid|).  p = 0 is an exact add.  The dropped fraction over
    2^20 + 37 elements lies within 5 sigma of p."""
    n = (1 << 20) + 37
    for k, seed in enumerate((0, 7, 0xFFFFFFFF)):
        x = _rand(n, 100 + k)
        x += 0.25 * torch.sign(x)          # |x| >= 0.25: a kept x / (1 - p) never rounds away against resid
        r = _rand(n, 200 + k) if with_resid else None
        y = torch.full((n,), float("nan"), device=dev)
        xd, rd = _dev(dev, x, r)
        _ok(lib.hirest_dropout_add_f32(_p(xd), _p(rd), _p(y), n, p, seed, _s()), "dropout_add")
        y = y.cpu()
        base = r if r is not None else torch.zeros(n)
        if p == 0.0:
            assert torch.equal(y, base + x)
            continue
        ks = torch.from_numpy(keep_scale(seed, np.arange(n, dtype=np.uint64), p))
        keep = ks != 0
        assert torch.equal(y != base, keep), f"seed {seed}: keep mask differs at {int((keep != (y != base)).sum())} elements"
        pf = float(np.float32(p))
        ref = base.double() + x.double() / (1.0 - pf)
        _within((y.double() - ref).abs()[keep], (4 * U * (x.double().abs() / (1 - pf) + base.double().abs()))[keep], f"dropout kept p={p}")
        frac = 1.0 - keep.double().mean().item()
        assert abs(frac - pf) <= 5 * np.sqrt(pf * (1 - pf) / n), (seed, frac)


def _gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / np.sqrt(2.0))


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_forward_and_backward(dev, lib, act):
    """n = 200 003 (not a multiple of the 256-thread block), x over [-30, 30] (erfc underflow, tanh saturation) plus random values.
    Forward: identity exact; tanh within 8 U |y| (a libm call of a few ulp); erf-GELU 0.5 x erfcf(fl(-x fl(1/sqrt 2))) within
    8 U |y| + 4 U x^2 phi(x): the argument carries 2 U of relative error (the constant and the product), which erfc's condition
    number turns into 2 U x^2 phi of absolute error in y (~200 U |y| at x = -10), doubled for margin.  On top, (|x| + 1) 2^-126
    absolute: an intermediate below the smallest normal float may flush to zero (erfc or phi = 0.399 exp(-x^2 / 2) near x = -13
    loses up to |x| 2^-126).  Backward against fp64 autograd, the same floor times (|dy| + 1):
      act 1: Phi + x phi.  phi = 0.399 __expf(-x^2 / 2): the fast exp's argument fl(fl(x x) / 2 * fl(log2 e)) carries three
             roundings, each U x^2 / 2 of absolute error in the exponent, plus the exp, the constant and the products: relative
             (1.5 x^2 + 8) U; Phi (erfc) within 8 U.  bar = |dy| (8 U Phi + (1.5 x^2 + 8) U |x phi|) + 2 U |dx| + floor;
      act 2: 1 - t^2 with t = tanhf(x) within 4 U: bar = |dy| 8 U + 2 U |dx|;
      act 3 (y = tanh(pre) given): 1 - y^2 in two roundings: bar = |dy| 4 U (1 + y^2) + 2 U |dx|;
      act 0: exact."""
    n = 200003
    x = torch.cat([torch.linspace(-30, 30, 100001), torch.tensor([0.0, -0.0, 30.0, -30.0, 1e-20, -1e-20]), _rand(n - 100007, 7, std=4.0)])
    if act == 3:
        x = torch.tanh(x.double()).float()
    dy = _rand(n, 8)
    xd, dyd = x.to(dev), dy.to(dev)
    x64 = x.double().requires_grad_(True)
    y64 = {0: lambda t: t, 1: _gelu64, 2: torch.tanh, 3: lambda t: t}[act](x64)
    tiny = (x.double().abs() + 1) * 2.0 ** -126
    if act <= 2:
        y = torch.full((n,), float("nan"), device=dev)
        _ok(lib.hirest_act_f32(_p(xd), _p(y), n, act, _s()), "act")
        y = y.cpu().double()
        if act == 0:
            assert torch.equal(y, x.double())
        else:
            a = x.double()
            arg = 4 * U * a * a * torch.exp(-0.5 * a * a) / np.sqrt(2 * np.pi) if act == 1 else 0.0
            _within((y - y64.detach()).abs(), 8 * U * y64.detach().abs() + arg + tiny, f"act {act} forward", at=x)
    dx = torch.full((n,), float("nan"), device=dev)
    _ok(lib.hirest_act_bwd_f32(_p(xd), _p(dyd), _p(dx), n, act, _s()), "act_bwd")
    dx = dx.cpu().double()
    if act == 3:
        ref = dy.double() * (1 - x.double() ** 2)
    else:
        y64.backward(dy.double())
        ref = x64.grad
    a, d = x.double(), dy.double().abs()
    tiny = tiny * (d + 1)
    if act == 0:
        assert torch.equal(dx, dy.double())
        return
    if act == 1:
        Phi = 0.5 * torch.special.erfc(-a / np.sqrt(2.0))
        xphi = (a * torch.exp(-0.5 * a * a) / np.sqrt(2 * np.pi)).abs()
        bar = d * (8 * U * Phi + (1.5 * a * a + 8) * U * xphi) + 2 * U * ref.abs() + tiny
    elif act == 2:
        bar = d * 8 * U + 2 * U * ref.abs() + tiny
    else:
        bar = d * 4 * U * (1 + a * a) + 2 * U * ref.abs() + tiny
    _within((dx - ref).abs(), bar, f"act {act} backward", at=x)


def test_scale_by_device_scalar(dev, lib):
    """x *= *scalar: one fp32 product, exact against torch's fp32 product (block tails at n = 1, 255, 257, 100 003)."""
    for n in (1, 255, 257, 100003):
        x = _rand(n, n)
        s = torch.tensor([-1.7], dtype=torch.float32)
        xd, sd = _dev(dev, x, s)
        _ok(lib.hirest_scale_by_device_scalar_f32(_p(xd), _p(sd), n, _s()), "scale_by_device_scalar")
        assert torch.equal(xd.cpu(), x * s)


@pytest.mark.parametrize("R,C,ld,Rp", [(1, 1, 1, 1), (1, 1, 3, 16), (31, 33, 40, 48), (33, 100, 100, 33), (100, 31, 35, 128), (65, 64, 64, 80)])
def test_transpose_pad(dev, lib, R, C, ld, Rp):
    """out[c][r] = in[r][c] for r < R, 0 for R <= r < Rp: exact, every element of out written (NaN-filled before)."""
    x = _rand((R, ld), R * 1000 + C)
    out = torch.full((C, Rp), float("nan"), device=dev)
    xd, = _dev(dev, x)
    _ok(lib.hirest_transpose_pad_f32(_p(xd), ld, R, C, _p(out), Rp, _s()), "transpose_pad")
    out = out.cpu()
    assert torch.equal(out[:, :R], x[:, :C].t())
    assert torch.equal(out[:, R:], torch.zeros(C, Rp - R))


# ---- reductions --------------------------------------------------------------------------------------------------------------------
# (R, D, eps): D in {384, 512, 768, 1024} runs the register forms, anything else the generic kernel; R not a multiple of the 4 rows
# of a block.  The last row of every case with R > 1 is constant (zero variance: xhat = 0, rstd = 1 / sqrt(eps)).
LN_CASES = [(1, 384, 1e-12), (5, 512, 1e-5), (3, 768, 1e-12), (1501, 1024, 1e-5), (1501, 768, 1e-5),
            (1, 64, 1e-5), (5, 100, 1e-12), (3, 767, 1e-5), (1501, 769, 1e-12), (5, 2048, 1e-5), (3, 2048, 1e-12)]


@pytest.mark.parametrize("R,D,eps", LN_CASES)
def test_layernorm_bwd(dev, lib, R, D, eps):
    """dx against fp64 autograd of F.layer_norm within 1e-5 of the row's max |dx|: the row statistics and the two projections
    (mean g, mean g xhat) are fp32 sums of D <= 2048 terms, D / 64 <= 32 per lane and 6 butterfly levels (~40 U ~ 2.4e-6 each),
    a few of them composed.  Column sums of dyxhat and dy (fp64 here) are dgamma and dbeta within 1e-5 of the column's
    sum of |terms|.  (Unbiased variance would move rstd by 1 / (2 (D - 1)) >= 2.4e-4 at D = 2048.)"""
    x = _rand((R, D), R + D, std=1.5, mean=0.3)
    if R > 1:
        x[-1] = 1.25                       # exact in every partial sum: mean exactly 1.25, variance exactly 0
    dy = _rand((R, D), R + D + 1)
    gamma = _rand(D, R + D + 2, std=0.1, mean=1.0)
    dx = torch.full((R, D), float("nan"), device=dev)
    dyx = torch.full((R, D), float("nan"), device=dev)
    xd, dyd, gd = _dev(dev, x, dy, gamma)
    _ok(lib.hirest_layernorm_bwd_f32(_p(xd), _p(dyd), _p(gd), eps, _p(dx), _p(dyx), R, D, _s()), "layernorm_bwd")
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (D,), g64, b64, float(np.float32(eps))).backward(dy.double())
    _rows_close(dx.cpu(), x64.grad, 1e-5, f"layernorm dx R={R} D={D}")
    dyx = dyx.cpu().double()
    mean = x.double().mean(-1, keepdim=True)
    xhat = (x.double() - mean) / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + float(np.float32(eps)))
    colscale = (dy.double() * xhat).abs().sum(0)
    _within((dyx.sum(0) - g64.grad).abs(), 1e-5 * colscale + 1e-30, f"layernorm dgamma R={R} D={D}")
    assert torch.allclose(dy.double().sum(0), b64.grad)


@pytest.mark.parametrize("R,C,ld,weighted,selected", [(7, 100, 103, True, False), (32, 33, 40, False, True), (33, 31, 31, True, True),
                                                       (1500, 768, 770, True, False), (300, 1, 3, False, False), (129, 257, 260, True, True)])
def test_weighted_colsum(dev, lib, R, C, ld, weighted, selected):
    """out[c] = sum_r w(r) [sel(r) == 1] x[r][c] against fp64.  Summation depth: R serial terms in the thin form (R <= 32), at most
    R / 128 + 2 per chain and 33 in the cross-lane sum in the wide form, so (R / 32 + 40) * 2 U * sum |w x| bounds both."""
    x = _rand((R, ld), R * 7 + C)
    w = _rand(R, R * 7 + C + 1) if weighted else None
    sel = _randint(0, 3, (R,), R + C) if selected else None
    out = torch.full((C,), float("nan"), device=dev)
    xd, wd, sd = _dev(dev, x, w, sel)
    _ok(lib.hirest_weighted_colsum_f32(_p(xd), ld, _p(wd), _p(sd), 1, R, C, _p(out), _s()), "weighted_colsum")
    wr = torch.ones(R, dtype=torch.float64) if w is None else w.double()
    if sel is not None:
        wr = wr * (sel == 1).double()
    terms = wr[:, None] * x[:, :C].double()
    _within((out.cpu().double() - terms.sum(0)).abs(), (R / 32 + 40) * 2 * U * terms.abs().sum(0) + 1e-300, f"colsum R={R} C={C}")


def test_joint_base_bwd(dev, lib):
    """Backward of feats = v * tn[:, None, :] against fp64 autograd at T around the 48-row unroll (1, 47, 48, 49, 97, 300) and
    E around the 256-thread block (1, 63, 64, 65, 255, 257, 768).  dv = dbase * tn is one fp32 product: exact.  dtn = sum_t dbase v is
    one fma chain of T terms: within (T + 1) U sum_t |dbase v|."""
    B = 2
    for T in (1, 47, 48, 49, 97, 300):
        for E in (1, 63, 64, 65, 255, 257, 768):
            db, v, tn = _rand((B, T, E), T * E), _rand((B, T, E), T * E + 1), _rand((B, E), T * E + 2, std=0.05)
            dv = torch.full((B, T, E), float("nan"), device=dev)
            dtn = torch.full((B, E), float("nan"), device=dev)
            dbd, vd, tnd = _dev(dev, db, v, tn)
            _ok(lib.hirest_joint_base_bwd_f32(_p(dbd), _p(vd), _p(tnd), _p(dv), _p(dtn), B, T, E, _s()), "joint_base_bwd")
            v64, t64 = v.double().requires_grad_(True), tn.double().requires_grad_(True)
            (v64 * t64[:, None, :]).backward(db.double())
            assert torch.equal(dv.cpu(), db * tn[:, None, :]), (T, E)
            assert torch.equal(dv.cpu().double(), v64.grad.float().double()), (T, E)
            _within((dtn.cpu().double() - t64.grad).abs(), (T + 1) * U * (db.double() * v.double()).abs().sum(1) + 1e-300,
                    f"joint_base_bwd dtn T={T} E={E}")


@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 257, 768])
def test_l2norm_bwd(dev, lib, E):
    """Backward of tn = t / |t| against fp64 autograd.  Two fp32 sums of E terms (E / 64 per lane + 6 levels) and a few products:
    within 1e-5 of the row scale (|dtn|_inf + |dtn|_2 |tn|_inf) / |t|, which bounds every term of (dtn - tn (tn . dtn)) / |t|."""
    B = 3
    t, dtn = _rand((B, E), E, std=2.0), _rand((B, E), E + 1)
    dt = torch.full((B, E), float("nan"), device=dev)
    td, dtnd = _dev(dev, t, dtn)
    _ok(lib.hirest_l2norm_bwd_f32(_p(td), _p(dtnd), _p(dt), B, E, _s()), "l2norm_bwd")
    t64 = t.double().requires_grad_(True)
    (t64 / t64.norm(dim=-1, keepdim=True)).backward(dtn.double())
    tn = t.double() / t.double().norm(dim=-1, keepdim=True)
    d = dtn.double()
    scale = (d.abs().amax(-1) + d.norm(dim=-1) * tn.abs().amax(-1)) / t.double().norm(dim=-1)
    _within((dt.cpu().double() - t64.grad).abs(), 1e-5 * scale[:, None].expand(B, E), f"l2norm_bwd E={E}")


@pytest.mark.parametrize("nheads", [1, 2, 3])
def test_heads_bwd(dev, lib, nheads):
    """dfeats = sum_h dl_h w_h^T, the input gradient of nheads Linear(D, 1) heads, against fp64 autograd: a product and up to
    two fmas, within 4 U sum_h |dl_h w_h|."""
    for rows in (1, 47, 600):
        for D in (1, 63, 65, 768):
            dl = _rand(nheads * rows, rows + D)
            ws = [_rand(D, rows + D + 1 + h) for h in range(nheads)]
            dld, *wd = _dev(dev, dl, *ws, *([None] * (3 - nheads)))
            out = torch.full((rows, D), float("nan"), device=dev)
            _ok(lib.hirest_heads_bwd_f32(_p(dld), rows, D, nheads, _p(wd[0]), _p(wd[1]), _p(wd[2]), _p(out), _s()), "heads_bwd")
            feats = torch.zeros((rows, D), dtype=torch.float64, requires_grad=True)
            logits = torch.stack([feats @ w.double() for w in ws])
            logits.backward(dl.double().reshape(nheads, rows))
            scale = sum((dl.double().reshape(nheads, rows)[h][:, None] * ws[h].double()[None, :]).abs() for h in range(nheads))
            _within((out.cpu().double() - feats.grad).abs(), 4 * U * scale + 1e-300, f"heads_bwd h={nheads} rows={rows} D={D}")


def test_embedding_forward_and_backward(dev, lib):
    """out[r] = table[ids[r]] + pos[r % T] (and pos[pos_ids[r]]): one fp32 add, exact.  Backward: dtable += index_add(ids, dx)
    with atomics in any order, within (n_id + 1) U (|dtable_0| + sum |dx|) of fp64, n_id = the number of rows of that id
    (37 ids over 900 rows: ~24 repeats each)."""
    V, T, B, D, P = 37, 300, 3, 100, 50
    rows = B * T
    ids = _randint(0, V, (rows,), 1)
    pos_ids = _randint(0, P, (rows,), 2)
    table, pos, pos2 = _rand((V, D), 3), _rand((T, D), 4), _rand((P, D), 5)
    out = torch.full((rows, D), float("nan"), device=dev)
    idd, pidd, tabd, posd, pos2d = _dev(dev, ids, pos_ids, table, pos, pos2)
    _ok(lib.hirest_embedding_fwd_f32(_p(idd), _p(tabd), _p(posd), _p(out), rows, T, D, _s()), "embedding_fwd")
    assert torch.equal(out.cpu(), table[ids.long()] + pos.repeat(B, 1))
    out.fill_(float("nan"))
    _ok(lib.hirest_embedding_pos_fwd_f32(_p(idd), _p(pidd), _p(tabd), _p(pos2d), _p(out), rows, D, _s()),
        "embedding_pos_fwd")
    assert torch.equal(out.cpu(), table[ids.long()] + pos2[pos_ids.long()])
    dx, d0 = _rand((rows, D), 6), _rand((V, D), 7)
    acc, dxd = _dev(dev, d0, dx)
    _ok(lib.hirest_embedding_bwd_f32(_p(idd), _p(dxd), _p(acc), rows, D, _s()), "embedding_bwd")
    ref = d0.double().index_add(0, ids.long(), dx.double())
    absum = d0.double().abs().index_add(0, ids.long(), dx.double().abs())
    cnt = torch.bincount(ids.long(), minlength=V).double()[:, None]
    _within((acc.cpu().double() - ref).abs(), (cnt + 1) * U * absum + 1e-300, "embedding_bwd")


# ---- losses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vr,V", [(5, 5), (5, 16), (255, 255), (257, 272), (30522, 30528)])
def test_ce_rows(dev, lib, Vr, V):
    """CrossEntropyLoss(ignore_index=-1) over R = 41 rows of V logits, row stride ld = V + 5 (NaN between V and ld: never read),
    the columns from Vr on at -3e38 as train.py pads the LM head; rows with target -1; weight 0.7 into a loss accumulator at 1.25.
    Against fp64 autograd: dlogits within 1e-5 of weight / n_valid (each is one softmax term: the exp of a difference of at most
    ~30 has ~30 U relative error, the row sum of V terms over 256 lanes ~ (V / 256 + 8) U); the loss within 1e-5 of the sum of
    |per-row terms| (each row's lse - x_t carries the same errors; 41 atomic adds in any order)."""
    R, ld, w, acc0 = 41, V + 5, 0.7, 1.25
    x = torch.full((R, ld), float("nan"))
    x[:, :V] = -3.0e38
    x[:, :Vr] = _rand((R, Vr), V, std=2.0)
    tg = _randint(0, Vr, (R,), V + 1)
    tg[::5] = -1
    n_valid = int((tg >= 0).sum())
    loss = torch.tensor([acc0], device=dev)
    dl = torch.full((R, ld), 123.0, device=dev)
    xd, tgd = _dev(dev, x, tg)
    _ok(lib.hirest_ce_rows_f32(_p(xd), ld, _p(tgd), R, V, w, n_valid, _p(loss), _p(dl), _s()), "ce_rows")
    x64 = x[:, :V].double().requires_grad_(True)
    terms = F.cross_entropy(x64, tg.long(), ignore_index=-1, reduction="none")
    (w * terms.sum() / n_valid).backward()
    ref = acc0 + w * terms.detach().sum().item() / n_valid
    assert abs(loss.item() - ref) <= 1e-5 * (acc0 + w * terms.detach().abs().sum().item() / n_valid), (loss.item(), ref)
    dl = dl.cpu()
    assert torch.equal(dl[:, V:], torch.full((R, ld - V), 123.0)), "dlogits written beyond V"
    assert torch.equal(dl[tg < 0, :V], torch.zeros(int((tg < 0).sum()), V))
    _within((dl[:, :V].double() - x64.grad).abs(), torch.full((R, V), 1e-5 * w / n_valid), f"ce_rows dlogits V={V}")


def _ce_masked_case(T, seed):
    """Rows: one frame; the whole row (target first, last); ALL ZERO; a span with the target at its start, at its end."""
    g = np.random.RandomState(seed)
    a = int(g.randint(0, T))
    b = int(g.randint(a, T))
    spans = [(T // 2, T // 2, T // 2), (0, T - 1, 0), (0, T - 1, T - 1), None, (a, b, a), (a, b, b)]
    B = len(spans)
    mask = torch.zeros((B, T), dtype=torch.int32)
    tg = torch.zeros(B, dtype=torch.int32)
    for i, sp in enumerate(spans):
        if sp is None:
            tg[i] = T // 3
            continue
        mask[i, sp[0]:sp[1] + 1] = 1
        tg[i] = sp[2]
    return mask, tg


def _ce_masked_run(dev, lib, x, mask, tg, w, acc0):
    B, T = x.shape
    loss = torch.tensor([acc0], device=dev)
    dl = torch.full((B, T), float("nan"), device=dev)
    xd, md, tgd = _dev(dev, x, mask, tg)
    _ok(lib.hirest_ce_masked_f32(_p(xd), _p(md), _p(tgd), B, T, w, _p(loss), _p(dl), _s()), "ce_masked")
    return loss.item(), dl.cpu()


@pytest.mark.parametrize("T", [1, 63, 64, 65, 300, 571])
def test_ce_masked(dev, lib, T):
    """modeling.py:343-344 in fp64: logits[mask == 0] = -finfo(float32).max, then F.cross_entropy (mean over B), times weight 0.6
    into an accumulator at 0.5.  An all-zero mask row is log(T), as torch gives.  dlogits (0 on masked frames: the in-place fill
    cuts them) within 1e-5 of weight / B, the loss within 1e-5 of the sum of |row terms| (the same per-row errors as ce_rows,
    over T <= 571 frames in one wave)."""
    w, acc0 = 0.6, 0.5
    mask, tg = _ce_masked_case(T, T)
    B = mask.shape[0]
    x = _rand((B, T), T, std=2.0)
    got, dl = _ce_masked_run(dev, lib, x, mask, tg, w, acc0)
    x64 = x.double().requires_grad_(True)
    xm = x64.masked_fill(mask == 0, -FMAX)
    terms = F.cross_entropy(xm, tg.long(), reduction="none")
    assert abs(terms[3].item() - np.log(T)) < 1e-12           # the all-zero row
    (w * terms.mean()).backward()
    ref = acc0 + w * terms.detach().mean().item()
    assert abs(got - ref) <= 1e-5 * (acc0 + w * terms.detach().abs().mean().item()), (got, ref)
    assert torch.equal(dl[mask == 0], torch.zeros(int((mask == 0).sum())))
    _within((dl.double() - x64.grad).abs(), torch.full((B, T), 1e-5 * w / B), f"ce_masked dlogits T={T}")


def test_ce_masked_target_outside_the_mask(dev, lib):
    """A target on a masked frame: torch's fp32 loss of that sample is finfo.max (its log-probability is -finfo.max), so the mean
    is finfo.max / B; the kernel must give the same within 1e-6 (fp32 reference).  The gradient stays finite: weight * softmax / B
    on the frames of the mask (fp64 autograd, within 1e-5 of weight / B)."""
    T, w = 300, 0.5
    mask = torch.zeros((2, T), dtype=torch.int32)
    mask[0, 10:41] = 1
    mask[1, 100:200] = 1
    tg = torch.tensor([5, 150], dtype=torch.int32)
    x = _rand((2, T), 77, std=2.0)
    got, dl = _ce_masked_run(dev, lib, x, mask, tg, w, 0.0)
    ref32 = w * F.cross_entropy(x.masked_fill(mask == 0, -FMAX), tg.long()).item()
    assert np.isfinite(got) and abs(got - ref32) <= 1e-6 * abs(ref32), (got, ref32)
    x64 = x.double().requires_grad_(True)
    (w * F.cross_entropy(x64.masked_fill(mask == 0, -FMAX), tg.long())).backward()
    _within((dl.double() - x64.grad).abs(), torch.full((2, T), 1e-5 * w / 2), "ce_masked dlogits, target outside")


@pytest.mark.parametrize("B,T,zero_mask", [(1, 1, False), (3, 50, False), (4, 64, False), (5, 300, False), (2, 200, True)])
def test_bce_masked(dev, lib, B, T, zero_mask):
    """modeling.py:249-263 in fp64: bce_with_logits(x, onehot(target)) * mask, summed, over max(sum mask, 1), times weight 0.5 into
    an accumulator at 0.25; B * T below, at and above the 256 threads of the one block.  The stable form's exp / log1p of |x| <= ~12
    carry ~(|x| + 2) 2 U ~ 2e-6 relative: dlogits within 1e-5 of weight / denominator, the loss within 1e-5 of the sum of |terms|.
    An all-zero mask adds exactly 0 and gives zero gradients."""
    w, acc0 = 0.5, 0.25
    x = _rand((B, T), B * T, std=3.0)
    tg = _randint(0, T, (B,), B * T + 1)
    mask = torch.zeros((B, T), dtype=torch.int32)
    if not zero_mask:
        for b in range(B):
            lo = int(tg[b]) // 2
            mask[b, lo:lo + T // 2 + 1] = 1
    loss = torch.tensor([acc0], device=dev)
    dl = torch.full((B, T), float("nan"), device=dev)
    xd, tgd, md = _dev(dev, x, tg, mask)
    _ok(lib.hirest_bce_masked_f32(_p(xd), _p(tgd), _p(md), B, T, w, _p(loss), _p(dl), _s()), "bce_masked")
    dl = dl.cpu()
    if zero_mask:
        assert loss.item() == acc0 and torch.equal(dl, torch.zeros(B, T))
        return
    x64 = x.double().requires_grad_(True)
    y = torch.zeros((B, T), dtype=torch.float64).scatter_(1, tg.long()[:, None], 1.0)
    m = mask.double()
    denom = m.sum().clamp(min=1)
    terms = F.binary_cross_entropy_with_logits(x64, y, reduction="none") * m
    (w * terms.sum() / denom).backward()
    ref = acc0 + w * terms.detach().sum().item() / denom.item()
    assert abs(loss.item() - ref) <= 1e-5 * (acc0 + w * terms.detach().abs().sum().item() / denom.item()), (loss.item(), ref)
    _within((dl.double() - x64.grad).abs(), torch.full((B, T), 1e-5 * w / denom.item()), f"bce_masked dlogits B={B} T={T}")


# ---- matrix products -----------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1), (31, 33, 63), (65, 200, 33), (200, 63, 65), (33, 1, 200), (1, 65, 31), (63, 31, 1)]


def _operand(rows, inner, contiguous_k, kind, seed, dev):
    """A [rows][inner] operand laid out k-contiguous (stride (ld, 1)) or rows-contiguous (stride (1, ld)).  kind 'vec': ld a
    multiple of 4 and an aligned base (the 16-byte load path); 'odd': ld not a multiple of 4; 'offset': the base one float past
    an aligned address.  Returns (device buffer, element offset, stride of rows, stride of k, the logical fp32 matrix); the pad
    between the logical extent and ld holds NaN, which must never reach the result."""
    major, minor = (rows, inner) if contiguous_k else (inner, rows)
    if kind == "odd":
        ld = minor + 1 if (minor + 1) % 4 else minor + 2
    else:
        ld = (minor + 3) // 4 * 4 + 4
    off = 1 if kind == "offset" else 0
    m = _rand((rows, inner), seed)
    buf = torch.full((off + major * ld,), float("nan"))
    view = buf[off:].view(major, ld)
    view[:, :minor] = m if contiguous_k else m.t()
    return buf.to(dev), off, (ld, 1) if contiguous_k else (1, ld), m


@pytest.mark.parametrize("a_kc", [True, False], ids=["A_kc", "A_mc"])
@pytest.mark.parametrize("b_kc", [True, False], ids=["B_kc", "B_nc"])
@pytest.mark.parametrize("kind", ["vec", "odd", "offset"])
def test_gemm_f32_strided(dev, lib, a_kc, b_kc, kind):
    """C = alpha A B^T (alpha = -0.75) over the four stride layouts, 16-byte and element-wise operand loads, M, N, K across the
    64 x 64 tile and the 32-deep slab (1, 31, 33, 63, 65, 200), C with row stride N + 3 (the pad must stay untouched).  Against
    fp64 elementwise within the n-term fp32 dot-product bound (K + 2) U |alpha| (|A| |B|^T)."""
    alpha = -0.75
    for i, (M, N, K) in enumerate(GEMM_SHAPES):
        A, aoff, (sam, sak), a = _operand(M, K, a_kc, kind, 10 * i + 1, dev)
        Bb, boff, (sbn, sbk), b = _operand(N, K, b_kc, kind, 10 * i + 2, dev)
        ldc = N + 3
        Cd = torch.full((M, ldc), 7.0, device=dev)
        _ok(lib.hirest_gemm_f32_strided(_p(A, aoff), sam, sak, _p(Bb, boff), sbn, sbk, _p(Cd), ldc, M, N, K, alpha, _s()), "gemm_f32_strided")
        Cd = Cd.cpu()
        assert torch.equal(Cd[:, N:], torch.full((M, 3), 7.0)), "C written beyond N"
        ref = alpha * a.double() @ b.double().t()
        bar = (K + 2) * U * abs(alpha) * (a.double().abs() @ b.double().abs().t())
        _within((Cd[:, :N].double() - ref).abs(), bar, f"gemm_f32_strided {kind} M={M} N={N} K={K}")


# ---- attention that keeps its probabilities -----------------------------------------------------------------------------------------
@pytest.fixture(params=[0, 1], ids=["rows", "tiled"])
def attn_impl(request, lib):
    _ok(lib.hirest_attention_train_select(request.param), "attention_train_select")
    yield request.param
    _ok(lib.hirest_attention_train_select(1), "attention_train_select")


def _attn_mask(B, Tq, Tk, seed):
    """Additive [B, Tq, Tk]: -10000 on future keys (j > i + Tk - Tq, key 0 always visible) and on padded keys (j >= len_b >= 1)."""
    lens = _randint(1, Tk + 1, (B,), seed)
    lens[0] = Tk
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    m = torch.zeros((B, Tq, Tk))
    for b in range(B):
        m[b][((j > i + (Tk - Tq)) & (j > 0)) | (j >= int(lens[b]))] = -10000.0
    return m


def _attn_ref(q, k, v, dctx, mask, keep, B, Tq, Tk, H, scale, addc):
    """fp64 autograd of ctx = (softmax(S) * keep) V, S = q k^T scale + (addc + mask).  With addc != 0 the scores are rounded as
    the kernel documents, S = fl(fl(q.k scale) + fl(addc + mask)) (a straight-through rounding: the gradient is the exact one)."""
    q64 = q.double().reshape(B, Tq, H, 64).permute(0, 2, 1, 3).requires_grad_(True)
    k64 = k.double().reshape(B, Tk, H, 64).permute(0, 2, 1, 3).requires_grad_(True)
    v64 = v.double().reshape(B, Tk, H, 64).permute(0, 2, 1, 3).requires_grad_(True)
    s = q64 @ k64.transpose(-1, -2) * scale
    add = torch.full((B, 1, Tq, Tk), addc, dtype=torch.float64)
    if mask is not None:
        add = add + mask.double()[:, None]
    S = s + add
    if addc != 0.0:
        S = S + ((s.detach().float() + add.float()).double() - S.detach())
    S.retain_grad()
    P = torch.softmax(S, -1)
    ctx = (P * keep) @ v64
    ctx.backward(dctx.double().reshape(B, Tq, H, 64).permute(0, 2, 1, 3))
    flat = lambda t, T: t.detach().permute(0, 2, 1, 3).reshape(B * T, H * 64)
    return P.detach(), flat(ctx, Tq), S.grad, flat(q64.grad, Tq), flat(k64.grad, Tk), flat(v64.grad, Tk)


def _attn_compare(got, ref, tol, what):
    """rows: a score row of P and dS, the 64 dimensions of one head of ctx, dq, dk and dv"""
    for name, g, r in zip(("P", "ctx", "dS", "dq", "dk", "dv"), got, ref):
        _rows_close(g.reshape(-1, r.shape[-1] if name in ("P", "dS") else 64), r.reshape(-1, r.shape[-1] if name in ("P", "dS") else 64),
                    tol, f"attention {name} {what}")


# (B, H, Tq, Tk, packed qkv, mask, dropout p)
ATTN_CASES = [(1, 1, 1, 1, True, False, 0.0), (2, 3, 1, 65, False, True, 0.1), (1, 2, 33, 31, False, True, 0.1),
              (3, 12, 48, 300, False, True, 0.1), (2, 12, 300, 300, True, False, 0.1), (1, 2, 129, 571, False, True, 0.0),
              (1, 2, 129, 571, False, False, 0.5)]


def _attn_run(dev, lib, B, H, Tq, Tk, packed, use_mask, p, addc, seed):
    D = H * 64
    scale = 0.125
    if packed:
        qkv = _rand((B * Tq, 3 * D), seed)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        qd = kd = qkv.to(dev)
        qo, ko, vo, ldq, ldkv = 0, D, 2 * D, 3 * D, 3 * D
    else:
        q, kv = _rand((B * Tq, D), seed), _rand((B * Tk, 2 * D), seed + 1)
        k, v = kv[:, :D], kv[:, D:]
        qd, kd = q.to(dev), kv.to(dev)
        qo, ko, vo, ldq, ldkv = 0, 0, D, D, 2 * D
    mask = _attn_mask(B, Tq, Tk, seed + 2) if use_mask else None
    dctx = _rand((B * Tq, D), seed + 3)
    dseed = 1000 + seed
    P = torch.full((B, H, Tq, Tk), float("nan"), device=dev)
    ctx = torch.full((B * Tq, D), float("nan"), device=dev)
    maskd, dctxd = _dev(dev, mask, dctx)
    _ok(lib.hirest_attention_train_fwd_qkv_f32(_p(qd, qo), ldq, _p(kd, ko), _p(kd, vo), ldkv, _p(maskd),
                                               _p(P), _p(ctx), D, B, Tq, Tk, H, 64, scale, addc, p, dseed, _s()), "attention_train_fwd_qkv")
    dS = torch.full((B, H, Tq, Tk), float("nan"), device=dev)
    if packed:
        dqkv = torch.full((B * Tq, 3 * D), float("nan"), device=dev)
        dq_, dk_, dv_, lddq, lddkv = (dqkv, 0), (dqkv, D), (dqkv, 2 * D), 3 * D, 3 * D
    else:
        dqb = torch.full((B * Tq, D), float("nan"), device=dev)
        dkv = torch.full((B * Tk, 2 * D), float("nan"), device=dev)
        dq_, dk_, dv_, lddq, lddkv = (dqb, 0), (dkv, 0), (dkv, D), D, 2 * D
    _ok(lib.hirest_attention_train_bwd_qkv_f32(_p(qd, qo), ldq, _p(kd, ko), _p(kd, vo), ldkv, _p(P), _p(dctxd), D, _p(dS), _p(*dq_), lddq,
                                               _p(*dk_), _p(*dv_), lddkv, B, Tq, Tk, H, 64, scale, p, dseed, _s()), "attention_train_bwd_qkv")
    got = [P.cpu(), ctx.cpu(), dS.cpu()]
    if packed:
        dqkv = dqkv.cpu()
        got += [dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]]
    else:
        dkv = dkv.cpu()
        got += [dqb.cpu(), dkv[:, :D], dkv[:, D:]]
    # dropout mask at element ((b H + h) Tq + i) Tk + j
    keep = torch.from_numpy(keep_scale(dseed, np.arange(B * H * Tq * Tk, dtype=np.uint64), p)).double().view(B, H, Tq, Tk)
    ref = _attn_ref(q, k, v, dctx, mask, keep, B, Tq, Tk, H, scale, addc)
    return got, ref


@pytest.mark.parametrize("B,H,Tq,Tk,packed,use_mask,p", ATTN_CASES)
def test_attention_train_vs_fp64(dev, lib, attn_impl, B, H, Tq, Tk, packed, use_mask, p):
    """P, ctx, dS, dq, dk, dv of both implementations against fp64 autograd, add_const = 0 (masked scores then sit at -10000 and
    vanish in the exp in both; unmasked ones get +0: no extra rounding).  Every output is a sum of at most 571 products of
    fp32 operands (scores: 64-deep) or a softmax row of them: within 1e-5 of the row's scale (row = the last dimension: a
    score row of P / dS, the 64 dimensions of one head of ctx / dq / dk / dv)."""
    got, ref = _attn_run(dev, lib, B, H, Tq, Tk, packed, use_mask, p, 0.0, B * 1000 + Tq * 10 + Tk)
    _attn_compare(got, ref, 1e-5, f"({B},{H},{Tq},{Tk}) p={p} impl={attn_impl}")


def test_attention_train_uniform_add_const(dev, lib, attn_impl):
    """add_const = -10000 (the all-zeros encoder mask): the reference rounds the scaled score to fp32 and adds the constant in fp32
    as the kernel does.  The kernel's fp32 score differs from the exact one by ~1e-6, which can flip that rounding to the next
    multiple of ulp(10000) = 2^-10, moving P by a factor exp(+-2^-10) and its row sum likewise: bar 2^-9 of the row scale."""
    got, ref = _attn_run(dev, lib, 2, 12, 300, 300, True, False, 0.1, -10000.0, 4242)
    _attn_compare(got, ref, 2.0 ** -9, f"add_const -10000 impl={attn_impl}")
