"""The kernels the towers, retrieval and beam search run around their GEMMs (csrc/elementwise.hip, csrc/score.hip), one entry point
at a time, against float64 torch / numpy on the CPU, at the shapes where row and tile kernels go wrong: every LayerNorm
instantiation and its round-up, D straddling a 256-column step, leading dimensions wider than the row, the bulk kernel's tail
rows and switch-over, grid-stride loops, second tiles of the similarity kernel, ragged and empty pooling segments, top-k rows
shorter than a wave, rows of -inf / +inf / one value, and the two-pass top-k with a short last chunk.

Bars (U = 2^-24, the fp32 unit roundoff; each docstring derives its own from the kernel's operation order):
  * data movement, casts, integer work, fp32 single operations that the CPU repeats exactly, top-k: bit equality;
  * sums taken in double and rounded once: one fp32 ulp;
  * fp32 sums: depth * U * sum |terms| (depth = serial terms per lane + butterfly levels), propagated per row / per element;
  * a bf16 output of a value y with fp32 error bar e must lie between bf16(ref - e) and bf16(ref + e) (rounding is monotonic),
    which pins all but the few elements whose reference lies within e of a rounding midpoint to one bf16 value.
Where an existing test applies a tighter constant to the same entry point (2e-5 LayerNorm at sigma 2, 2e-6 pooling, 1e-5
similarity), the smaller of the two is used.  Output buffers are wider / longer than what the kernel should write and filled
with NaN first: what lies outside must still be NaN.  Refused argument combinations are exercised on the CPU only
(tests/test_abi_and_host.py); every call here is a valid one.

Each group was run once against a library built with one mutation (MI355X; failed / selected tests):
  launch_ln rounds NV 9..12 down to 8                    test_layernorm_rows D = 2052, 2304, 3072, both types (6 / 28): unwritten columns
  layernorm_rows_bulk stores its tail rows unguarded     test_layernorm_bulk, all five D (the NaN rows behind 8193 / 8207 rows)
  ln_wave_stats divides by D - 1                         every LayerNorm value test (43 / 43; the row_index test compares the kernel
                                                         with itself and cannot see it)
  rowstats: statistics of the unrounded row              test_rowstats_* 17 / 18
  ln_finalize reads g < G - G % 8                        test_ln_stats_finalize groups 1, 7, 9, 44 (16 / 20; groups = 8 is unaffected)
  fold_layernorm sums W gamma unrounded                  test_fold_layernorm 8 / 8
  patchify swaps dy and dx                               test_patchify_* 23 / 23
  patchify uint8 u * (1 / 255.f)                         none, rightly: 325 of the 768 fp32 values change, none of their bf16 roundings
                                                         (the precondition the uint8 test asserts says so for any fp32 order)
  embed_tokens tie rule oi > bi                          test_embed_tokens, every L > 1 (8 / 10)
  pool_l2 divides by F - 1                               the F = 1 cases and the one-row segments (7 / 16: 0 / 0); for F > 1 the final
                                                         L2 normalisation removes any scale of the mean, the outputs are the same
  similarity loads only v <= V - 2                       test_similarity* 6 / 6
  topk_chunk writes index 0 for missing candidates       none: equivalent.  Such a slot carries score -inf and the smallest tie key, so
                                                         it loses to every real candidate, and the chunks always hold >= k real ones
  better() with ta < tb                                  test_topk_exact 18 / 18
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 67


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


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, std=1.0, mean=0.0):
    return torch.randn(shape, generator=_gen(seed), dtype=torch.float64).mul_(std).add_(mean).float()


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def _strided(t, ld, junk):
    """t [R, D] as the leading columns of a [R, ld] matrix whose other columns hold `junk`."""
    R, D = t.shape
    m = torch.full((R, ld), junk, dtype=t.dtype)
    m[:, :D] = t
    return m


def _nan_out(dev, rows, ld, dtype=torch.float32):
    """[rows, ld] output plus PAD trailing elements, all NaN."""
    return torch.full((rows * ld + PAD,), float("nan"), dtype=dtype, device=dev)


def _split_out(buf, rows, ld, D, what):
    """The written [rows, D] part of a NaN-filled [rows, ld] (+ PAD) buffer; everything else must still be NaN."""
    buf = buf.cpu()
    assert torch.isnan(buf[rows * ld:]).all(), f"{what}: written past row {rows - 1}"
    m = buf[:rows * ld].view(rows, ld)
    assert torch.isnan(m[:, D:]).all(), f"{what}: written into the padding columns"
    body = m[:, :D]
    assert not torch.isnan(body.float()).any(), f"{what}: elements left unwritten"
    return body


def _within(err, bar, what):
    err, bar = err.double(), bar.double()
    assert not torch.isnan(err).any(), f"{what}: NaN"
    r = (err / bar.clamp_min(1e-300)).flatten()
    ratio = r.max().item() if r.numel() else 0.0
    print(f"{what}: worst err/bar {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: err/bar {ratio:.3g} at flat index {int(r.argmax())}"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _bf16_between(got, ref, e, what):
    """got (bf16) = bf16(y') for some |y' - ref| <= e: bf16(ref - e) <= got <= bf16(ref + e), rounding being monotonic.  The fp64
    bounds pass through fp32 on their way to bf16; widening e by U |ref| covers that rounding."""
    e = e + U * ref.abs() + 1e-300
    lo = (ref - e).float().to(torch.bfloat16).double()
    hi = (ref + e).float().to(torch.bfloat16).double()
    g = got.double()
    bad = ((g < lo) | (g > hi) | torch.isnan(g)).nonzero()
    pinned = (lo == hi).double().mean().item()
    print(f"{what}: {pinned * 100:.2f} % of the elements pinned to one bf16 value")
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} bf16 outputs outside [bf16(ref - e), bf16(ref + e)], first at {bad[0].tolist()}"


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def _ln_nv(D):
    nv = (D // 4 + 63) // 64
    return nv if nv <= 8 else (12 if nv <= 12 else 16 if nv <= 16 else 24 if nv <= 24 else 32)


def _ln_ref_bar(x, g, b, eps, nv):
    """fp64 LayerNorm (biased variance) of x [R, D] and the per-element bound on the fp32 two-pass form's error.
    A lane adds nv groups of four (a two-level tree each) and the wave a six-level butterfly: the row sum has depth ds = nv + 8,
    so the mean is off by em <= ds U sum|x| / D + U |mean| (the division).  d = x - mean then carries U |d| + em, the sum of
    squares (depth dq = 4 nv + 6, one rounding for the square) (dq + 1) U sum d^2 + 2 sum |d| (U |d| + em); with the division by D
    dvar <= (dq + 4) U var + 2 em mean|d|.  var + eps, the square root and the reciprocal add at most 4 U to half of that:
    er = dvar / (2 (var + eps)) + 4 U is the relative error of rstd.  y = (d rstd) g + b: three roundings of the product's
    magnitude at most (subtract, multiply, multiply; two when the last is fused), em rstd |g| from the mean, one rounding of y:
      |y - ref| <= |g| rstd (em + |d| (3 U + er)) + U |ref|,   times 1.01 for the second-order terms."""
    D = x.shape[1]
    x64, g64, b64 = x.double(), g.double(), b.double()
    mean = x64.mean(1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = d * rstd * g64 + b64
    ds, dq = nv + 8, 4 * nv + 6
    em = ds * U * x64.abs().sum(1, keepdim=True) / D + U * mean.abs()
    dvar = (dq + 4) * U * var + 2 * em * d.abs().mean(1, keepdim=True)
    er = dvar / (2 * (var + eps)) + 4 * U
    bar = 1.01 * (g64.abs() * rstd * (em + d.abs() * (3 * U + er)) + U * ref.abs())
    return ref, bar


def _ln_params(D, seed):
    return _rand((D,), seed, std=0.2, mean=1.0), _rand((D,), seed + 1, std=0.2)


def _run_ln(dev, lib, xs, ldx, g, b, eps, rows, D, ldo, f32, row_index=None):
    """xs: device [*, ldx]; returns the NaN-checked [rows, D] output (CPU).  Four more NaN rows follow the output (one wave's
    group of rows in the bulk kernel) and must stay NaN."""
    out = _nan_out(dev, rows + 4, ldo, torch.float32 if f32 else torch.bfloat16)
    _ok(lib.hirest_layernorm(_p(xs), ldx, _p(row_index), _p(g), _p(b), eps, _p(out), ldo, 1 if f32 else 0, rows, D, _s()), "layernorm")
    torch.cuda.synchronize()
    return _split_out(out, rows, ldo, D, f"layernorm rows={rows} D={D} f32={f32}")


LN_D = [4, 252, 256, 260, 1024, 1280, 1792, 2048, 2052, 2304, 3072, 4096, 4100, 8192]


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_rows(dev, lib, D, f32):
    """The per-row kernel at every instantiation NV = 1..8, 12, 16, 24, 32 (D = 4 .. 8192; 2052, 2304 and 3072 take the round-up
    9 -> 12 and 12, 4100 the round-up 17 -> 24), D on both sides of a 256-column step, rows 1, 3, 5 (a partly filled block of four
    waves) and 301, ldx = D + 4, ldo = D + 8, against fp64 with the bar of _ln_ref_bar.  The data is the existing LayerNorm test's
    (sigma 2, mean 0.3, gamma 1 +- 0.2), so its 2e-5 absolute bar applies too: the smaller of the two is used.  bf16 output: between
    the bf16 roundings of ref -+ that bar."""
    eps = 1e-5
    g, b = _ln_params(D, D)
    gd, bd = g.to(dev), b.to(dev)
    for rows in (1, 3, 5, 301):
        x = _rand((rows, D), D * 7 + rows, std=2.0, mean=0.3)
        xs = _strided(x, D + 4, 1e30).to(dev)
        got = _run_ln(dev, lib, xs, D + 4, gd, bd, eps, rows, D, D + 8, f32)
        ref, bar = _ln_ref_bar(x, g, b, eps, _ln_nv(D))
        bar = bar.clamp_max(2e-5)
        if f32:
            _within((got.double() - ref).abs(), bar, f"layernorm f32 rows={rows} D={D}")
        else:
            _bf16_between(got, ref, bar, f"layernorm bf16 rows={rows} D={D}")


def _edge_rows(x, at_const, at_offset, seed):
    """Overwrites rows `at_const` with the constant 1.5 and rows `at_offset` with mean 1e3, sigma 1."""
    D = x.shape[1]
    for i, r in enumerate(at_const):
        x[r] = 1.5
    for i, r in enumerate(at_offset):
        x[r] = _rand((D,), seed + i, std=1.0, mean=1000.0)
    return x


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [4, 260, 1408, 3072, 8192])
def test_layernorm_value_edges(dev, lib, D, f32):
    """Two rows where a LayerNorm goes wrong.  A constant row of 1.5: every partial sum k * 1.5 (k <= 8192) is an fp32 number, so
    the mean is 1.5 exactly, x - mean = 0, and the output is beta exactly (bf16(beta) for bf16 output), whatever rstd is.  A row of
    mean 1e3 and sigma 1: the two-pass form keeps the bar of _ln_ref_bar (here about 1e-3 |gamma|: the mean itself is only good to
    (nv + 9) U 1e3); the one-pass E[x^2] - mean^2 in fp32 would lose U 1e6 = 0.06 of a variance of 1."""
    eps = 1e-5
    g, b = _ln_params(D, D + 50)
    rows = 6
    x = _edge_rows(_rand((rows, D), D + 51, std=2.0, mean=0.3), [1, 5], [0, 4], D + 52)
    xs = _strided(x, D + 4, 1e30).to(dev)
    got = _run_ln(dev, lib, xs, D + 4, g.to(dev), b.to(dev), eps, rows, D, D + 8, f32)
    ref, bar = _ln_ref_bar(x, g, b, eps, _ln_nv(D))
    want_b = b if f32 else b.to(torch.bfloat16)
    for r in (1, 5):
        assert torch.equal(_bits(got[r]), _bits(want_b)), f"constant row {r}: output is not beta exactly"
    keep = [0, 2, 3, 4]
    if f32:
        _within((got.double() - ref).abs()[keep], bar[keep], f"layernorm edges f32 D={D}")
    else:
        _bf16_between(got[keep], ref[keep], bar[keep], f"layernorm edges bf16 D={D}")


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [260, 1408, 4100])
def test_layernorm_row_index_bit_equal(dev, lib, D, f32):
    """row_index (repeated and permuted source rows, written to consecutive output rows) gives the bits of the plain call on those
    rows, for both output types: the gather changes the address of a row and nothing else."""
    eps, R = 1e-6, 23
    g, b = _ln_params(D, D + 60)
    x = _rand((R, D), D + 61, std=2.0, mean=0.3)
    xs = _strided(x, D + 4, 1e30).to(dev)
    gd, bd = g.to(dev), b.to(dev)
    plain = _run_ln(dev, lib, xs, D + 4, gd, bd, eps, R, D, D + 8, f32)
    idx = torch.tensor([22, 0, 7, 7, 3, 22, 11, 1, 0], dtype=torch.int32)
    got = _run_ln(dev, lib, xs, D + 4, gd, bd, eps, idx.numel(), D, D + 8, f32, row_index=idx.to(dev))
    assert torch.equal(_bits(got), _bits(plain[idx.long()]))


@pytest.mark.parametrize("D", [256, 512, 1024, 1280, 1536])
def test_layernorm_bulk(dev, lib, D):
    """The bulk kernel (bf16 output, no row_index, rows >= 8192, D <= 1536: four rows per wave, grid-strided) at NV = 1, 2, 4, 5, 6,
    ldx = D + 4, ldo = D + 8, with 8192, 8193 and 8207 rows: the last wave's group of four is full, holds one row, holds three.  Rows
    past the end must stay NaN (a tail that wrote its clamped source row anywhere would either overwrite row rows - 1's neighbour or
    leave the true tail rows unwritten).  The same buffer with 8191 rows goes through the per-row kernel; both are held to fp64 with
    the same bar, not to each other (the bulk kernel sums zeros for the columns past D and may fuse differently: its depth is not
    larger).  Rows 5 / 8200 are constant (output bf16(beta) exactly), rows 6 / 8201 have mean 1e3, sigma 1."""
    eps, R = 1e-6, 8207
    g, b = _ln_params(D, D + 70)
    x = _edge_rows(_rand((R, D), D + 71, std=2.0, mean=0.3), [5, 8200], [6, 8201], D + 72)
    xs = _strided(x, D + 4, 1e30).to(dev)
    gd, bd = g.to(dev), b.to(dev)
    ref, bar = _ln_ref_bar(x, g, b, eps, _ln_nv(D))
    normal = torch.ones(R, dtype=torch.bool)
    normal[[5, 6, 8200, 8201]] = False
    bar[normal] = bar[normal].clamp_max(2e-5)
    bb = _bits(b.to(torch.bfloat16))
    for rows in (8191, 8192, 8193, 8207):
        got = _run_ln(dev, lib, xs, D + 4, gd, bd, eps, rows, D, D + 8, False)
        for r in (5, 8200):
            if r < rows:
                assert torch.equal(_bits(got[r]), bb), f"rows={rows}: constant row {r} is not beta exactly"
        keep = torch.ones(rows, dtype=torch.bool)
        keep[5] = False
        if rows > 8200:
            keep[8200] = False
        _bf16_between(got[keep], ref[:rows][keep], bar[:rows][keep], f"layernorm {'bulk' if rows >= 8192 else 'per-row'} rows={rows} D={D}")


# ---- LN-fold statistics -----------------------------------------------------------------------------------------------------------
def _stats_ref_bar(f64, eps, depth):
    """(mean, rstd) in fp64 of rows f64 and the bounds for sums S, Q taken in fp32 with depth `depth` and finished in double:
    dS <= depth U sum|f|, dQ <= depth U sum f^2 (the squares are fused into the accumulation: one rounding per step);
    mean = fl(S / D): dS / D + U |mean|;  var = Q / D - mean^2: dvar <= dQ / D + 2 |mean| dS / D;  rstd = fl(1 / sqrt(var + eps)):
    rstd (dvar / (2 (var + eps)) + U).  1.01 for the second-order terms."""
    D = f64.shape[1]
    mean = f64.mean(1)
    var = ((f64 - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    dS = depth * U * f64.abs().sum(1) / D
    dQ = depth * U * (f64 * f64).sum(1) / D
    bar_mean = 1.01 * (dS + U * mean.abs())
    bar_rstd = 1.01 * rstd * ((dQ + 2 * mean.abs() * dS) / (2 * (var + eps)) + U)
    return mean, rstd, bar_mean, bar_rstd


def _guard_ref_bar(mean, rstd, bar_mean, bar_rstd):
    ratio = mean.abs() * rstd
    bar = bar_mean * rstd + mean.abs() * bar_rstd + U * ratio           # the product of the two fp32 statistics, one rounding
    return ratio.max().item(), bar.max().item()


@pytest.mark.parametrize("rows", [1, 5, 16390])
@pytest.mark.parametrize("D", [4, 256, 260, 1408, 1536])
def test_rowstats_split(dev, lib, D, rows):
    """hirest_rowstats_split_bf16 at NV = 1, 2, 6 and both sides of the 256-column step, ldx = D + 4, 16390 rows = six more than
    the 16384 waves of the capped grid (the grid-stride loop).  xb must be x.to(bfloat16) and xlo (x - xb.float()).to(bfloat16), bit
    for bit (one fp32 subtraction, exact on both sides).  stats are those of the ROUNDED row: a lane adds 4 NV <= 24 values and
    squares serially, the wave six levels: depth 4 NV + 6 in _stats_ref_bar.  The guard must equal max |mean| rstd over the rows
    within the bound that follows from the two; a guard already above that value keeps its bits."""
    eps = 1e-6
    x = _rand((rows, D), D * 3 + rows, std=2.0, mean=0.3)
    xs = _strided(x, D + 4, 1e30).to(dev)
    xb = torch.full((rows * D + PAD,), float("nan"), dtype=torch.bfloat16, device=dev)
    xlo = torch.full((rows * D + PAD,), float("nan"), dtype=torch.bfloat16, device=dev)
    stats = torch.full((rows * 2 + PAD,), float("nan"), dtype=torch.float32, device=dev)
    guard = torch.zeros(1, dtype=torch.float32, device=dev)
    _ok(lib.hirest_rowstats_split_bf16(_p(xs), D + 4, _p(xb), _p(xlo), _p(stats), eps, rows, D, _p(guard), _s()), "rowstats_split")
    torch.cuda.synchronize()
    hi = _split_out(xb, rows, D, D, "rowstats xb")
    lo = _split_out(xlo, rows, D, D, "rowstats xlo")
    st = _split_out(stats, rows, 2, 2, "rowstats stats")
    want_hi = x.to(torch.bfloat16)
    assert torch.equal(_bits(hi), _bits(want_hi)), "xb is not bf16(x)"
    assert torch.equal(_bits(lo), _bits((x - want_hi.float()).to(torch.bfloat16))), "xlo is not bf16(x - xb)"
    nv = (D // 4 + 63) // 64
    mean, rstd, bm, br = _stats_ref_bar(want_hi.double(), eps, 4 * nv + 6)
    _within((st[:, 0].double() - mean).abs(), bm, f"rowstats mean rows={rows} D={D}")
    _within((st[:, 1].double() - rstd).abs(), br, f"rowstats rstd rows={rows} D={D}")
    gref, gbar = _guard_ref_bar(mean, rstd, bm, br)
    gval = guard.item()
    print(f"rowstats guard {gval:.6g} ref {gref:.6g} err/bar {abs(gval - gref) / gbar:.3g}")
    assert abs(gval - gref) <= gbar
    # a larger value already there stays; without xlo (hirest_rowstats_bf16) xb and the statistics are the same bits
    high = torch.tensor([gref * 2 + 1], dtype=torch.float32)
    guard2 = high.to(dev)
    xb2 = torch.full((rows * D + PAD,), float("nan"), dtype=torch.bfloat16, device=dev)
    stats2 = torch.full((rows * 2 + PAD,), float("nan"), dtype=torch.float32, device=dev)
    _ok(lib.hirest_rowstats_bf16(_p(xs), D + 4, _p(xb2), _p(stats2), eps, rows, D, _p(guard2), _s()), "rowstats")
    torch.cuda.synchronize()
    assert torch.equal(_bits(guard2.cpu()), _bits(high)), "a guard above the rows' maximum was changed"
    assert torch.equal(_bits(_split_out(xb2, rows, D, D, "rowstats xb (no xlo)")), _bits(want_hi))
    assert torch.equal(_bits(_split_out(stats2, rows, 2, 2, "rowstats stats (no xlo)")), _bits(st))


@pytest.mark.parametrize("D,rows,bad", [(4, 1, 0), (260, 5, 3), (1408, 16390, 16389)])
def test_rowstats_guard_trips_on_nan_row(dev, lib, D, rows, bad):
    """One row holding a NaN (first, middle, the last row of the grid-stride loop's second trip) raises the guard to +inf - fmaxf
    alone would drop it - and leaves every other row's statistics within their bars; guard NULL is accepted."""
    eps = 1e-6
    x = _rand((rows, D), D + rows, std=2.0, mean=0.3)
    x[bad, D // 2] = float("nan")
    xs = _strided(x, D + 4, 1e30).to(dev)
    xb = torch.empty((rows, D), dtype=torch.bfloat16, device=dev)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=dev)
    guard = torch.zeros(1, dtype=torch.float32, device=dev)
    _ok(lib.hirest_rowstats_bf16(_p(xs), D + 4, _p(xb), _p(stats), eps, rows, D, _p(guard), _s()), "rowstats")
    torch.cuda.synchronize()
    assert guard.item() == float("inf")
    st = stats.cpu()
    good = torch.ones(rows, dtype=torch.bool)
    good[bad] = False
    if good.any():
        mean, rstd, bm, br = _stats_ref_bar(x[good].to(torch.bfloat16).double(), eps, 4 * ((D // 4 + 63) // 64) + 6)
        _within((st[good, 0].double() - mean).abs(), bm, "rowstats mean beside a NaN row")
        _within((st[good, 1].double() - rstd).abs(), br, "rowstats rstd beside a NaN row")
    stats2 = torch.empty((rows, 2), dtype=torch.float32, device=dev)
    _ok(lib.hirest_rowstats_bf16(_p(xs), D + 4, _p(xb), _p(stats2), eps, rows, D, None, _s()), "rowstats guard=NULL")
    torch.cuda.synchronize()
    assert torch.equal(_bits(stats2.cpu()[good]), _bits(st[good]))


@pytest.mark.parametrize("rows", [1, 31, 33, 1000])
@pytest.mark.parametrize("groups", [1, 7, 8, 9, 44])
def test_ln_stats_finalize(dev, lib, groups, rows):
    """partials [rows, groups, 2] = fp32 (sum, sum of squares) of each 32-column group of random rows (D = 32 groups), a third of the
    rows with mean 50 sigma.  The kernel adds the partials in double (eight lanes a row, groups not a multiple of eight leave lanes
    idle; rows not a multiple of 32 leave a block partly filled), so against fp64 sums of the same fp32 partials only the final
    roundings remain: mean U |mean|; var = Q / D - mean^2 in double loses 2^-53 (Q / D + mean^2) - times 8 for the order of the adds
    and the reference's own rounding - and rstd one fp32 rounding: rstd (U + 8 2^-53 (Q / D + mean^2) / (2 (var + eps)))."""
    eps = 1e-6
    D = 32 * groups
    x = _rand((rows, D), groups * 1000 + rows, std=2.0, mean=0.3).double()
    x[::3] += 100.0                                                     # mean 50 sigma
    xg = x.view(rows, groups, 32)
    part = torch.stack([xg.sum(2), (xg * xg).sum(2)], dim=2).float()    # the input of the kernel: fp32 partials
    pd = part.to(dev)
    stats = torch.full((rows * 2 + PAD,), float("nan"), dtype=torch.float32, device=dev)
    guard = torch.zeros(1, dtype=torch.float32, device=dev)
    _ok(lib.hirest_ln_stats_finalize(_p(pd), groups, _p(stats), eps, rows, D, _p(guard), _s()), "ln_stats_finalize")
    torch.cuda.synchronize()
    st = _split_out(stats, rows, 2, 2, "finalize stats")
    S, Q = part[:, :, 0].double().sum(1), part[:, :, 1].double().sum(1)
    mean = S / D
    var = (Q / D - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    bm = 1.01 * U * mean.abs() + 1e-300
    br = 1.01 * rstd * (U + 8 * 2.0 ** -53 * (Q / D + mean * mean) / (2 * (var + eps)))
    _within((st[:, 0].double() - mean).abs(), bm, f"finalize mean groups={groups} rows={rows}")
    _within((st[:, 1].double() - rstd).abs(), br, f"finalize rstd groups={groups} rows={rows}")
    gref, gbar = _guard_ref_bar(mean, rstd, bm, br)
    assert abs(guard.item() - gref) <= gbar, (guard.item(), gref, gbar)
    high = torch.tensor([gref * 2 + 1], dtype=torch.float32)
    guard2 = high.to(dev)
    _ok(lib.hirest_ln_stats_finalize(_p(pd), groups, _p(stats), eps, rows, D, _p(guard2), _s()), "ln_stats_finalize")
    torch.cuda.synchronize()
    assert torch.equal(_bits(guard2.cpu()), _bits(high)), "a guard above the rows' maximum was changed"


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("N,K", [(1, 4), (5, 70), (130, 1408), (64, 4096)])
def test_fold_layernorm(dev, lib, N, K, with_bias):
    """Wf = bf16(W gamma) with the product formed in fp32: one multiplication and one conversion, which the CPU repeats exactly ->
    bit equality.  colsum_out[n] = sum_k float(Wf[n][k]) and bias_out[n] = bias[n] + sum_k W[n][k] beta[k] are summed in double
    (the products of two fp32 numbers are exact in double) and rounded once: within one fp32 ulp of the fp64 value, plus
    2^-50 sum |terms| for the order of the double additions.  N = 1, 5 and 130 leave the last block of four waves partly filled,
    K = 4 and 70 most lanes of a wave idle (K = 70 is not a multiple of 4 or 64)."""
    W = _rand((N, K), N * 10000 + K, std=0.05)
    gamma, beta = _rand((K,), K + 1, std=0.3, mean=1.0), _rand((K,), K + 2, std=0.3)
    bias = _rand((N,), N + 3, std=0.5) if with_bias else None
    Wd, gd, bd = W.to(dev), gamma.to(dev), beta.to(dev)
    biasd = bias.to(dev) if with_bias else None
    wf = torch.full((N * K + PAD,), float("nan"), dtype=torch.bfloat16, device=dev)
    bo = torch.full((N + PAD,), float("nan"), dtype=torch.float32, device=dev)
    so = torch.full((N + PAD,), float("nan"), dtype=torch.float32, device=dev)
    _ok(lib.hirest_fold_layernorm(_p(Wd), _p(gd), _p(bd), _p(biasd), _p(wf), _p(bo), _p(so), N, K, _s()), "fold_layernorm")
    torch.cuda.synchronize()
    got_wf = _split_out(wf, N, K, K, "fold Wf")
    want_wf = (W * gamma).to(torch.bfloat16)
    assert torch.equal(_bits(got_wf), _bits(want_wf)), "Wf is not bf16(W * gamma)"
    s_ref = want_wf.double().sum(1)
    s_abs = want_wf.double().abs().sum(1)
    prod = W.double() * beta.double()
    b_ref = prod.sum(1) + (bias.double() if with_bias else 0.0)
    b_abs = prod.abs().sum(1) + (bias.double().abs() if with_bias else 0.0)
    ulp = lambda r: torch.from_numpy(np.spacing(np.abs(r.float().numpy()))).double()
    _within((_split_out(so, N, 1, 1, "fold colsum")[:, 0].double() - s_ref).abs(), ulp(s_ref) + 2.0 ** -50 * s_abs, f"fold colsum N={N} K={K}")
    _within((_split_out(bo, N, 1, 1, "fold bias")[:, 0].double() - b_ref).abs(), ulp(b_ref) + 2.0 ** -50 * b_abs, f"fold bias N={N} K={K}")


@pytest.mark.parametrize("rows,D,stride_rows", [(37, 260, 1), (3, 1408, 257), (1, 4, 1), (6000, 1408, 1)])
def test_combine_hi_lo_bit_equal(dev, lib, rows, D, stride_rows):
    """out = float(hi) + float(lo): one fp32 addition -> bit equality.  ld_in = D + 4 with ldo = D + 8, and ld_in = 257 D (the
    tower's CLS rows: every 257th row of the residual stream, written to consecutive rows); 6000 x 1408 is more than the 8192 x 256
    threads of the capped grid (grid-stride loop)."""
    ld_in = D + 4 if stride_rows == 1 else stride_rows * D
    src_rows = (rows - 1) * stride_rows + 1
    hi = _rand((src_rows, D), rows + D, std=2.0).to(torch.bfloat16)
    lo = _rand((src_rows, D), rows + D + 1, std=2.0 ** -9).to(torch.bfloat16)
    if stride_rows == 1:
        hs, ls = _strided(hi, ld_in, 1e30).to(dev), _strided(lo, ld_in, 1e30).to(dev)
        want = hi.float() + lo.float()
    else:
        hs, ls = hi.to(dev), lo.to(dev)
        want = hi[::stride_rows].float() + lo[::stride_rows].float()
    out = _nan_out(dev, rows, D + 8)
    _ok(lib.hirest_combine_hi_lo_f32(_p(hs), _p(ls), ld_in, _p(out), D + 8, rows, D, _s()), "combine_hi_lo")
    torch.cuda.synchronize()
    got = _split_out(out, rows, D + 8, D, "combine_hi_lo")
    assert torch.equal(_bits(got), _bits(want))


# ---- patch extraction -------------------------------------------------------------------------------------------------------------
def _patch_ref(img, P):
    """img [B, 3, S, S] -> [B (S/P)^2, 3 P P], column (c, dy, dx), patch row (b, ph, pw)."""
    B, _, S, _ = img.shape
    G = S // P
    return img.reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * P * P)


def _run_patchify(dev, lib, frames, code, B, S, P, Kpad, mean=None, std=None):
    rows = B * (S // P) ** 2
    out = torch.full((rows * Kpad + PAD,), float("nan"), dtype=torch.bfloat16, device=dev)
    fd = frames.to(dev)
    md, sd = (None if mean is None else mean.to(dev)), (None if std is None else std.to(dev))
    _ok(lib.hirest_patchify(_p(fd), code, B, S, P, _p(md), _p(sd), _p(out), Kpad, _s()), "patchify")
    torch.cuda.synchronize()
    return _split_out(out, rows, Kpad, Kpad, f"patchify S={S} P={P} Kpad={Kpad} B={B}")


PATCH_CASES = [(224, 14, 640, 1), (224, 14, 640, 3), (224, 16, 768, 1), (224, 16, 768, 3), (224, 32, 3072, 1), (224, 32, 3072, 3),
               (32, 32, 3072, 1), (32, 32, 3072, 3), (28, 14, 592, 1), (28, 14, 592, 3), (224, 14, 640, 52)]


@pytest.mark.parametrize("in_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("S,P,Kpad,B", PATCH_CASES)
def test_patchify_exact(dev, lib, S, P, Kpad, B, in_bf16):
    """Pure data movement plus one conversion: patches[:, :3 P P] equals the reshaped image converted to bf16 bit for bit, for f32
    and bf16 NCHW input, and the columns from 3 P P to Kpad are exact zeros (the header's promise; the GEMM multiplies them).
    P = 14 / 16 / 32 with and without padding columns, S == P (one patch a frame), a 2 x 2 grid with Kpad = 592 (four padding
    columns, half a 16-byte store), and B = 52 at (224, 14, 640): 52 x 256 x 80 threads' worth of work for a grid capped at
    4096 x 256 (the grid-stride loop).  Every pixel has its own value (a random image), so a swapped dy / dx, channel or patch
    index cannot pass."""
    img = _rand((B, 3, S, S), S * 100 + P + B, std=1.2)
    if in_bf16:
        img = img.to(torch.bfloat16)
    got = _run_patchify(dev, lib, img, 1 if in_bf16 else 0, B, S, P, Kpad)
    K = 3 * P * P
    assert torch.equal(_bits(got[:, :K]), _bits(_patch_ref(img, P).to(torch.bfloat16)))
    assert torch.equal(_bits(got[:, K:]), torch.zeros_like(_bits(got[:, K:]))), "padding columns are not +0"


def _bf16_round_f64(v):
    """Round-to-nearest bf16 of fp64 values v != 0 (numpy) without passing through fp32, and the distance of v from the midpoint of
    the two bf16 numbers around it."""
    a = np.abs(v)
    ulp = 2.0 ** (np.floor(np.log2(a)) - 7)
    lo = np.floor(a / ulp) * ulp
    hi = lo + ulp
    mid = lo + ulp / 2
    r = np.where(a < mid, lo, hi)
    return np.sign(v) * r, np.abs(a - mid)


def test_patchify_uint8_exhaustive_bit_exact(dev, lib):
    """uint8 NHWC input with the fused (u / 255 - mean) / std: there are only 256 x 3 (level, channel) pairs, and the frames here
    hold all of them (pixel i of a 28 x 28 frame has level (i + 85 c + 7 b) mod 256 in channel c).  Every output must be the
    round-to-nearest bf16 of the fp64 value x of (u / 255 - mean) / std (mean, std: the fp32 numbers the kernel reads), bit for bit.
    That bar is derived, not measured: three fp32 roundings (quotient, difference, quotient) move the result by at most
      2^-24 ((u / 255 + |u / 255 - mean|) / std + |x|),
    and the test first asserts, on the host, that every one of the 768 values of x lies more than twice that far from the midpoint of
    its two bf16 neighbours (with CLIP's constants the smallest ratio is 10.9) - so no fp32 evaluation order can change the bf16
    result, and another mean / std for which that does not hold fails here instead of making the comparison vacuous."""
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float32)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float32)
    m, s = mean.double().numpy(), std.double().numpy()
    lv = np.arange(256, dtype=np.float64)[:, None] / 255.0
    xv = (lv - m) / s                                                   # [256, 3] fp64
    table, dist = _bf16_round_f64(xv)
    bound = 2.0 ** -24 * ((lv + np.abs(lv - m)) / s + np.abs(xv))
    ratio = (dist / bound).min()
    print(f"uint8 normalise: smallest (distance to a bf16 midpoint) / (fp32 error bound) = {ratio:.3g}")
    assert ratio > 2.0, "precondition of the bit-exact bar does not hold for this mean / std"
    B, S, P, Kpad = 3, 28, 14, 592
    i = np.arange(S * S).reshape(1, S, S, 1)
    u = ((i + 85 * np.arange(3).reshape(1, 1, 1, 3) + 7 * np.arange(B).reshape(B, 1, 1, 1)) % 256).astype(np.uint8)
    for c in range(3):
        assert len(np.unique(u[..., c])) == 256
    got = _run_patchify(dev, lib, torch.from_numpy(u), 2, B, S, P, Kpad, mean, std)
    want_img = torch.from_numpy(table[u.astype(np.int64), np.arange(3).reshape(1, 1, 1, 3)]).permute(0, 3, 1, 2)     # [B, 3, S, S] fp64, bf16 numbers
    want = _patch_ref(want_img, P).to(torch.bfloat16)
    assert torch.equal(want.double(), _patch_ref(want_img, P)), "the table holds bf16 numbers"
    K = 3 * P * P
    diff = (_bits(got[:, :K]) != _bits(want)).nonzero()
    assert diff.numel() == 0, f"{diff.shape[0]} outputs differ from bf16(fp64 value), first at {diff[0].tolist()}"
    assert torch.equal(_bits(got[:, K:]), torch.zeros_like(_bits(got[:, K:])))


# ---- CLS rows, token embedding, cast ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,D", [(1, 1, 4), (3, 50, 768), (3, 257, 1408), (1, 257, 768), (3, 1, 1408), (1, 50, 4), (2048, 2, 1408)])
def test_write_cls_rows(dev, lib, B, T, D):
    """x[b T, :D] = cls + pos0 (one fp32 addition, bit equality) for b < B with ldx = D + 4, and every other element of the NaN-filled
    buffer - the padding columns, the T - 1 rows between two CLS rows, the tail - untouched.  B = 2048 at D = 1408 is 2048 x 352
    threads' worth for a grid capped at 2048 x 256 (grid-stride loop)."""
    cls, pos0 = _rand((D,), D + B, std=0.5), _rand((D,), D + B + 1, std=0.5)
    ldx = D + 4
    x = _nan_out(dev, B * T, ldx)
    cd, pd = cls.to(dev), pos0.to(dev)
    _ok(lib.hirest_write_cls_rows(_p(x), ldx, _p(cd), _p(pd), B, T, D, _s()), "write_cls_rows")
    torch.cuda.synchronize()
    xc = x.cpu()
    assert torch.isnan(xc[B * T * ldx:]).all()
    m = xc[:B * T * ldx].view(B, T, ldx)
    assert torch.equal(_bits(m[:, 0, :D]), _bits((cls + pos0).expand(B, D)))
    assert torch.isnan(m[:, 0, D:]).all() and torch.isnan(m[:, 1:, :]).all(), "an element outside the CLS rows was written"


def _eot_tokens(L, vocab, seed):
    """Rows of token ids whose maximum is repeated at chosen positions (those that fit L), one row of equal ids, one row whose
    maximum is unique and last; other ids are below the maximum."""
    g = _gen(seed)
    rows, want = [], []
    for pos in ((0, 63), (1, 64, 65), (70, 76), (L - 1,), (0,), (63, 64)):
        if max(pos) >= L:
            continue
        t = torch.randint(0, vocab - 1, (L,), generator=g, dtype=torch.int64)
        t[list(pos)] = vocab - 1
        rows.append(t)
        want.append(min(pos))
    rows.append(torch.full((L,), 7, dtype=torch.int64))
    want.append(0)
    return torch.stack(rows), want


@pytest.mark.parametrize("D", [4, 512])
@pytest.mark.parametrize("L", [1, 5, 64, 77, 200])
def test_embed_tokens(dev, lib, L, D):
    """x[b, t] = tok_emb[clamp(id, 0, vocab - 1)] + pos[t] (one fp32 addition: bit equality) and eot_row[b] = b L + first position
    of the row's maximum id.  L = 1, L shorter than a wave, one wave, 77 and 200 (a lane sees up to four ids); the maximum repeated
    in lanes (0, 63), across the stride (1, 64, 65), late (70, 76), and a row of equal ids (position 0).  A second call holds ids
    outside the table (-5, -1, vocab, 2^40), which the kernel clamps; the argmax is over the ids as given, a row of negative ids
    included (its first maximum is -1 in the middle, not position 0).  eot_row = NULL leaves x the same.  B L is odd for most L (the last block of four waves is partly filled)."""
    vocab = 97
    emb, pos = _rand((vocab, D), L + D, std=0.5), _rand((L, D), L + D + 1, std=0.5)
    ed, pd = emb.to(dev), pos.to(dev)
    tok, want_eot = _eot_tokens(L, vocab, L * 31 + D)
    wild = tok.clone()
    wild[0, 0] = 2 ** 40
    wild[-1, :] = -5
    wild[-1, L // 2] = -1                                                  # the row's maximum, unique
    if L > 2:
        wild[1 % wild.shape[0], 2] = vocab                                # = vocab: clamps to the last row ...
    for t, eot_want in ((tok, want_eot), (wild, None)):
        B = t.shape[0]
        td = t.to(dev)
        x = _nan_out(dev, B * L, D)
        eot = torch.full((B + PAD,), -7, dtype=torch.int32, device=dev)
        _ok(lib.hirest_embed_tokens(_p(td), _p(ed), _p(pd), _p(x), _p(eot), B, L, D, vocab, _s()), "embed_tokens")
        torch.cuda.synchronize()
        got = _split_out(x, B * L, D, D, "embed_tokens x").view(B, L, D)
        want = emb[t.clamp(0, vocab - 1)] + pos[None]
        assert torch.equal(_bits(got), _bits(want))
        e = eot.cpu()
        assert (e[B:] == -7).all()
        first_max = torch.from_numpy(np.argmax(t.numpy(), axis=1))       # numpy: the first maximum
        assert torch.equal(e[:B].long(), torch.arange(B) * L + first_max)
        if eot_want is not None:
            assert first_max.tolist() == eot_want
        x2 = _nan_out(dev, B * L, D)
        _ok(lib.hirest_embed_tokens(_p(td), _p(ed), _p(pd), _p(x2), None, B, L, D, vocab, _s()), "embed_tokens eot=NULL")
        torch.cuda.synchronize()
        assert torch.equal(_bits(_split_out(x2, B * L, D, D, "embed_tokens x (eot NULL)").view(B, L, D)), _bits(want))


def test_f32_to_bf16_bit_equal(dev, lib):
    """Bit-equal to torch's CPU conversion (round to nearest even) on: ties that round down to an even and up to an even mantissa,
    values just beside them, +-0, the smallest and largest fp32 subnormals, the smallest normal, the largest finite fp32 and the
    largest value that still rounds to a finite bf16 (beyond it the result is inf), +-inf; NaN must stay NaN; then 2^21 + 12 random
    values, more than the 2048 x 256 x 4 elements of the capped grid (grid-stride loop)."""
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)
    edge_bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000,
                 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,
                 0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    edges = torch.from_numpy(f(edge_bits).copy())
    n_nan = 3
    x = torch.cat([edges, _rand((2 ** 21 + 12,), 99, std=3.0)])
    assert x.numel() % 4 == 0
    xd = x.to(dev)
    out = torch.full((x.numel() + PAD,), 1.0, dtype=torch.bfloat16, device=dev)
    _ok(lib.hirest_f32_to_bf16(_p(xd), _p(out), x.numel(), _s()), "f32_to_bf16")
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[x.numel():].float() == 1.0).all(), "written past n"
    got, want = o[:x.numel()], x.to(torch.bfloat16)
    nan = torch.isnan(x)
    assert int(nan.sum()) == n_nan and torch.isnan(got[nan].float()).all(), "NaN did not stay NaN"
    diff = (_bits(got)[~nan] != _bits(want)[~nan]).nonzero()
    assert diff.numel() == 0, f"{diff.shape[0]} differ, first at {diff[0].tolist()}: {x[~nan][diff[0]].item()!r}"


# ---- pooling ----------------------------------------------------------------------------------------------------------------------
def _pool_ref_bar(x, norm_first):
    """x [F, E] fp32 -> (fp64 L2-normalised mean, per-element bound).  Frame norms (norm_first): a lane squares and adds
    4 ceil(E / 256) values, the wave six levels: n is good to rn = (4 ceil(E / 256) + 7) / 2 U + U relative, the quotient adds U.
    The mean is a serial sum of F terms and one division: bm = (F - 1 + rq) U sum_f |x_f| / F + U |m| with rq the terms' own
    relative error in units of U.  |m|^2: a thread adds 4 ceil(E / 1024) squares, the wave six levels, four waves serially:
    depth dn = 4 ceil(E / 1024) + 10, and it inherits 2 sum |m| bm; the norm is good to rN = (dn + 1) U / 2 + sum |m| bm / |m|^2
    + U, and out = m / N to bm / N + |out| (rN + U).  1.01 for second-order terms."""
    F, E = x.shape
    x64 = x.double()
    rq = 0.0
    if norm_first:
        x64 = x64 / x64.norm(dim=1, keepdim=True)
        rq = (4 * -(-E // 256) + 7) / 2 + 2
    m = x64.mean(0)
    bm = (F - 1 + rq) * U * x64.abs().sum(0) / F + U * m.abs()
    N2 = (m * m).sum()
    N = torch.sqrt(N2)
    dn = 4 * -(-E // 1024) + 10
    rN = (dn + 1) * U / 2 + (m.abs() * bm).sum() / N2 + U
    ref = m / N
    return ref, 1.01 * (bm / N + ref.abs() * (rN + U))


@pytest.mark.parametrize("norm_first", [0, 1])
@pytest.mark.parametrize("V,F,E", [(1, 1, 4), (3, 1, 512), (5, 7, 1000), (2, 300, 2048), (1, 8192, 64)])
def test_pool_l2norm(dev, lib, V, F, E, norm_first):
    """One frame (plain L2), one thread active (E = 4), idle threads (E = 512, 64, 1000 = 250 float4), two trips (E = 2048), and
    F = 8192, the limit (dynamic LDS (F + 8) 4 bytes), against fp64 with the bar of _pool_ref_bar, capped by the existing test's 2e-6.
    Elements have mean 1 so that the mean over frames does not cancel: the bound's F U sum |x| / F term is then a relative one."""
    x = _rand((V, F, E), V * 1000 + F + E, std=1.0, mean=1.0)
    xd = x.to(dev)
    out = _nan_out(dev, V, E)
    _ok(lib.hirest_pool_l2norm(_p(xd), _p(out), V, F, E, norm_first, _s()), "pool_l2norm")
    torch.cuda.synchronize()
    got = _split_out(out, V, E, E, "pool_l2norm")
    for v in range(V):
        ref, bar = _pool_ref_bar(x[v], bool(norm_first))
        _within((got[v].double() - ref).abs(), bar.clamp_max(2e-6), f"pool_l2norm V={V} F={F} E={E} nf={norm_first} v={v}")


@pytest.mark.parametrize("E", [4, 384, 1028])
@pytest.mark.parametrize("lens", [[0, 1, 5, 0, 700, 1], [3, 0, 700, 2, 0]], ids=["empty-first-middle", "empty-last"])
def test_pool_l2norm_varlen(dev, lib, lens, E):
    """Ragged segments of a packed [rows, E] matrix: empty first, in the middle and last (exact zeros), one row (plain L2), 700 rows;
    E = 1028 is one float4 more than a trip of 256 threads.  Non-empty segments against fp64 with _pool_ref_bar, capped at 2e-6."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = int(off[-1])
    x = _rand((rows, E), rows + E, std=1.0, mean=1.0)
    xd, od = x.to(dev), torch.from_numpy(off).to(dev)
    V = len(lens)
    out = _nan_out(dev, V, E)
    _ok(lib.hirest_pool_l2norm_varlen(_p(xd), _p(od), _p(out), V, E, _s()), "pool_l2norm_varlen")
    torch.cuda.synchronize()
    got = _split_out(out, V, E, E, "pool_l2norm_varlen")
    for v, n in enumerate(lens):
        if n == 0:
            assert torch.equal(_bits(got[v]), torch.zeros(E, dtype=torch.int32)), f"empty segment {v} is not +0"
            continue
        ref, bar = _pool_ref_bar(x[off[v]:off[v + 1]], False)
        _within((got[v].double() - ref).abs(), bar.clamp_max(2e-6), f"pool varlen E={E} segment {v} ({n} rows)")


# ---- similarity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,V,E", [(1, 1, 4), (65, 64, 17), (64, 129, 1000), (130, 200, 1024), (3, 1000, 512)])
def test_similarity(dev, lib, Q, V, E):
    """One element, a second tile of queries (65), of videos (129, 200, 1000), both (130 x 200); E = 4, 17 and 1000 are not
    multiples of the 16-column step.  Each score is one serial chain of E fused multiply-adds: |err| <= E U sum_e |t_e v_e|,
    capped by the existing test's 1e-5 (rows are L2-normalised as in retrieval).  The NaN-filled output shows a tile that writes
    past V or Q."""
    t = torch.nn.functional.normalize(_rand((Q, E), Q + E, 1.0).double(), dim=1).float()
    vn = torch.nn.functional.normalize(_rand((V, E), V + E + 1, 1.0).double(), dim=1).float()
    td, vd = t.to(dev), vn.to(dev)
    out = _nan_out(dev, Q, V)
    _ok(lib.hirest_similarity_f32(_p(td), _p(vd), _p(out), Q, V, E, _s()), "similarity")
    torch.cuda.synchronize()
    got = _split_out(out, Q, V, V, "similarity")
    ref = t.double() @ vn.double().T
    bar = (E * U * (t.double().abs() @ vn.double().abs().T)).clamp_max(1e-5)
    _within((got.double() - ref).abs(), bar, f"similarity Q={Q} V={V} E={E}")


def test_similarity_identity_is_exact_transpose(dev, lib):
    """T = the E x E identity: S[q][v] = Vn[v][q] exactly (one product by 1, the rest zeros), an asymmetric 68 x 131 result that no
    swapped operand, shifted tile or dropped edge column can reproduce."""
    E, V = 68, 131
    vn = _rand((V, E), 5, 1.0)
    td, vd = torch.eye(E).to(dev), vn.to(dev)
    out = _nan_out(dev, E, V)
    _ok(lib.hirest_similarity_f32(_p(td), _p(vd), _p(out), E, V, E, _s()), "similarity")
    torch.cuda.synchronize()
    got = _split_out(out, E, V, V, "similarity identity")
    assert torch.equal(_bits(got), _bits(vn.T.contiguous()))


# ---- top-k ------------------------------------------------------------------------------------------------------------------------
def _topk_rows(V, k, seed):
    """Rows: scores quantised to 16 levels (many ties); half -inf; all -inf but min(3, V) (k above the number of finite scores
    whenever k > 3); three +inf; one repeated value."""
    g = _gen(seed)
    q = lambda: (torch.randint(0, 16, (V,), generator=g).float() - 8) / 4
    inf = float("inf")
    r0, r1, r2, r3 = q(), q(), torch.full((V,), -inf), q()
    r1[torch.randperm(V, generator=g)[:V // 2]] = -inf
    keep = torch.randperm(V, generator=g)[:min(3, V)]
    r2[keep] = q()[keep]
    r3[torch.randperm(V, generator=g)[:min(3, V)]] = inf
    return torch.stack([r0, r1, r2, r3, torch.full((V,), 0.25)])


@pytest.mark.parametrize("with_tie_rank", [True, False], ids=["tie_rank", "by-index"])
@pytest.mark.parametrize("V,k", [(1, 1), (5, 5), (63, 63), (255, 16), (257, 257), (12288, 10), (12289, 10), (16387, 10),
                                 (16384 + 4096 + 3, 16)])
def test_topk_exact(dev, lib, V, k, with_tie_rank):
    """Exact indices and scores against oracle.ref_cpu.topk_with_ties (score descending, then tie key descending; without tie_rank
    the key is the index), through hirest_topk_f32 and hirest_topk_f32_ws, which must agree.  k == V, V = 1, V below a wave and
    below a block, three chunks (12288: one pass, workspace NULL accepted) and four (12289: two passes, last chunk of 1 element;
    16387 and 20483: last chunk of 3 < k, whose empty candidate slots carry index -1 and must never be selected).  Every score is
    finite or +-inf; NaN is excluded by the header."""
    from oracle import ref_cpu as O
    scores = _topk_rows(V, k, V * 100 + k)
    Q = scores.shape[0]
    tie = torch.randperm(V, generator=_gen(V + k)).int() if with_tie_rank else None
    want = O.topk_with_ties(scores, tie if with_tie_rank else torch.arange(V, dtype=torch.int32), k)
    want_s = torch.gather(scores, 1, want)
    sd = scores.to(dev)
    tied = tie.to(dev) if with_tie_rank else None
    nchunk = (V + 4095) // 4096
    results = []
    for ws_form in (False, True):
        idx = torch.full((Q * k + PAD,), -7, dtype=torch.int32, device=dev)
        val = _nan_out(dev, Q, k)
        if not ws_form:
            _ok(lib.hirest_topk_f32(_p(sd), _p(tied), Q, V, k, _p(idx), _p(val), _s()), "topk")
        else:
            need = lib.hirest_topk_workspace_bytes(Q, V, k)
            assert need == Q * nchunk * k * 12
            ws = torch.empty(need, dtype=torch.uint8, device=dev) if nchunk >= 4 else None
            _ok(lib.hirest_topk_f32_ws(_p(sd), _p(tied), Q, V, k, _p(idx), _p(val), _p(ws), need if ws is not None else 0, _s()), "topk_ws")
        torch.cuda.synchronize()
        ic = idx.cpu()
        assert (ic[Q * k:] == -7).all()
        got_i = ic[:Q * k].view(Q, k).long()
        got_s = _split_out(val, Q, k, k, "topk scores")
        what = f"topk{'_ws' if ws_form else ''} V={V} k={k}"
        bad = (got_i != want).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} indices differ, first (row, rank) = {bad[0].tolist()}: " \
                                 f"{got_i[bad[0][0], bad[0][1]].item()} != {want[bad[0][0], bad[0][1]].item()}"
        assert torch.equal(got_s, want_s), f"{what}: scores differ"
        results.append(got_i)
        # index output alone (out_score NULL)
        idx2 = torch.full((Q * k,), -7, dtype=torch.int32, device=dev)
        if not ws_form:
            _ok(lib.hirest_topk_f32(_p(sd), _p(tied), Q, V, k, _p(idx2), None, _s()), "topk")
            torch.cuda.synchronize()
            assert torch.equal(idx2.cpu().view(Q, k).long(), want)
    assert torch.equal(results[0], results[1])
