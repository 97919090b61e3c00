"""The joint model's inference entry points (csrc/joint.hip, csrc/caption.hip), one at a time, against float64 torch on the CPU or
the reference's own CPU restatements (oracle.ref_cpu), at the shapes where kernels go wrong: row and column tails of every block,
ties across lanes, waves and strides, all-masked rows, the ends of the threshold walk, the 1-, 3- and 4-wave attention blocks, the
first and last step of a beam search.  Each test calls its entry point through _lib.load() the way moment_model.py, caption.hip
and sentence_encoder.py call it.

Bars (derived from the fp32 arithmetic of each operation, U = 2^-24 the fp32 unit roundoff; see each docstring):
  * integer, index, mask and bookkeeping work, the time grid, the beam search against RefBeam: exact;
  * elementwise kernels: a few roundings of the operands' magnitude;
  * sums: depth * U * sum |terms|, the depth being the kernel's summation depth (serial terms per lane + butterfly levels);
  * softmax-weighted sums: the relative error of every probability (score error, exp, row sum) times sum p |v|.
Every output buffer is allocated larger than the kernel should write and filled with a sentinel first: what lies outside the
written range must still hold it, what lies inside must have been overwritten.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # fp32 unit roundoff
FMAX = float(np.finfo(np.float32).max)
PAD = 67                       # sentinel elements behind every output


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
    return None if t is None else t.data_ptr() + t.element_size() * offset


def _rand(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).mul_(std).add_(mean).float()


def _dev(dev, *ts):
    """Device copies that stay referenced until the caller's launch."""
    return [None if t is None else t.to(dev) for t in ts]


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def _out(dev, n, fill=float("nan"), dtype=torch.float32):
    """An output of n elements followed by PAD sentinel elements."""
    return torch.full((n + PAD,), fill, dtype=dtype, device=dev)


def _body(buf, n, fill=float("nan"), what=""):
    """The first n elements (CPU); asserts that the PAD behind them still hold the sentinel."""
    buf = buf.cpu()
    tail = buf[n:]
    same = torch.isnan(tail).all() if isinstance(fill, float) and np.isnan(fill) else torch.equal(tail, torch.full_like(tail, fill))
    assert same, f"{what}: written past its {n} elements"
    return buf[:n]


def _within(err, bar, what):
    """err, bar: tensors of the same shape; prints the worst err / bar so that a run shows the margin."""
    err, bar = err.double(), bar.double()
    assert not torch.isnan(err).any(), f"{what}: NaN (an element left unwritten)"
    r = (err / bar.clamp_min(1e-300)).flatten()
    ratio = r.max().item() if r.numel() else 0.0
    print(f"{what}: worst err/bar {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: err/bar {ratio:.3g}"


# ---- fusion -----------------------------------------------------------------------------------------------------------------------
def test_time_grid_equals_cpu_linspace_bit_for_bit(dev, lib):
    """grid[b][t] = (torch.linspace(0, 1, n_b)[t] - 0.5) * 2 for t < n_b, else 0, with the reference's own CPU float32 call
    (modeling.py:184), bit for bit: every n_valid from 0 to T = 2048 in one launch (B = 2049 rows).  CPU linspace takes its upper
    half as 1 - (n - 1 - t) * step in one rounding; a separate multiply and subtract differs by one ulp for most n >= 10."""
    B, T = 2049, 2048
    nv = torch.arange(B, dtype=torch.int32)
    nvd, = _dev(dev, nv)
    grid = _out(dev, B * T)
    _ok(lib.hirest_joint_time_grid_f32(_p(nvd), B, T, _p(grid), _s()), "joint_time_grid")
    got = _body(grid, B * T, what="time grid").view(B, T)
    ref = torch.zeros((B, T), dtype=torch.float32)
    for n in range(1, B):
        ref[n, :n] = (torch.linspace(0, 1, n) - 0.5) * 2
    bad = (got.view(torch.int32) != ref.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} grid values differ, first (n, t) = {bad[0].tolist()}"


@pytest.mark.parametrize("E", [4, 512, 516])
def test_joint_time_features(dev, lib, E):
    """tin[b,t,:] = tanh(grid[b,t] w1 + b1) against fp64 on the kernel's own grid values (pinned bit for bit above).  The argument
    is one fused multiply-add (at most two roundings without contraction): 2 U (|g w1| + |b1|), which tanh (slope <= 1) passes on;
    tanhf itself within 4 ulp <= 8 U |y|; 2^-126 absolute for a subnormal flushed.  n_valid 0, 1, 171, 300 at T = 300."""
    B, T = 4, 300
    nv = torch.tensor([0, 1, 171, 300], dtype=torch.int32)
    w1, b1 = _rand(E, E, std=1.5), _rand(E, E + 1, std=0.5)
    nvd, w1d, b1d = _dev(dev, nv, w1, b1)
    grid = _out(dev, B * T)
    _ok(lib.hirest_joint_time_grid_f32(_p(nvd), B, T, _p(grid), _s()), "joint_time_grid")
    tin = _out(dev, B * T * E)
    _ok(lib.hirest_joint_time_features(_p(nvd), _p(w1d), _p(b1d), _p(tin), B, T, E, _s()), "joint_time_features")
    g = _body(grid, B * T).double().view(B, T, 1)
    got = _body(tin, B * T * E, what="time features").double().view(B, T, E)
    gw = g * w1.double()
    ref = torch.tanh(gw + b1.double())
    bar = 2 * U * (gw.abs() + b1.double().abs()) + 8 * U * ref.abs() + 2.0 ** -126
    _within((got - ref).abs(), bar, f"joint_time_features E={E}")


@pytest.mark.parametrize("E", [4, 512, 516, 1028])
def test_joint_base(dev, lib, E):
    """base = v (t / |t|) + asr + temporal against fp64, T around the 16-row block (1, 15, 16, 17, 300, 1855).  |t|^2 is bounded
    as an E-term fp32 sum (relative E U), the square root halves it and adds U, the quotient and the product one U each:
    |v tn| (E / 2 + 3) U; the two adds at most 2 U of the running magnitude: 2 U (|v tn| + |asr| + |temporal|)."""
    for T in (1, 15, 16, 17, 300, 1855):
        B = 5 if T <= 17 else 2
        s = T * 10000 + E
        v, t, a, tm = _rand((B, T, E), s), _rand((B, E), s + 1, std=2.0), _rand((B, T, E), s + 2), _rand((B, T, E), s + 3)
        vd, td, ad, tmd = _dev(dev, v, t, a, tm)
        base = _out(dev, B * T * E)
        _ok(lib.hirest_joint_base(_p(vd), _p(td), _p(ad), _p(tmd), _p(base), B, T, E, _s()), "joint_base")
        got = _body(base, B * T * E, what=f"joint_base T={T} E={E}").double().view(B, T, E)
        t64 = t.double()
        vt = v.double() * (t64 / t64.norm(dim=-1, keepdim=True))[:, None, :]
        ref = vt + a.double() + tm.double()
        bar = vt.abs() * (E / 2 + 3) * U + 2 * U * (vt.abs() + a.double().abs() + tm.double().abs()) + 1e-300
        _within((got - ref).abs(), bar, f"joint_base T={T} E={E}")


@pytest.mark.parametrize("with_boundary", [True, False], ids=["boundary", "no-boundary"])
def test_joint_mask_add_exact(dev, lib, with_boundary):
    """f = (base + boundary_embed[bm]) + mask_embed[mm], the kernel's documented order, exactly as float32 torch evaluates it; with
    boundary_mask NULL f = base + mask_embed[mm].  Both embedding rows are used, the first and last rows of the call included."""
    for rows, E in ((1, 4), (602, 516), (5, 1028)):
        base = _rand((rows, E), rows + E)
        me, be = _rand((2, E), rows + E + 1), _rand((2, E), rows + E + 2)
        g = torch.Generator().manual_seed(rows)
        mm = torch.randint(0, 2, (rows,), generator=g, dtype=torch.int32)
        bm = torch.randint(0, 2, (rows,), generator=g, dtype=torch.int32)
        mm[0], mm[-1] = 1, 0
        bm[0], bm[-1] = 0, 1
        if rows > 2:
            mm[1], bm[1] = 0, 1
        bd, mmd, bmd, med, bed = _dev(dev, base, mm, bm, me, be)
        f = _out(dev, rows * E)
        _ok(lib.hirest_joint_mask_add(_p(bd), _p(mmd), _p(bmd) if with_boundary else None, _p(med), _p(bed) if with_boundary else None,
                                      _p(f), rows, E, _s()), "joint_mask_add")
        got = _body(f, rows * E, what="joint_mask_add").view(rows, E)
        ref = ((base + be[bm.long()]) + me[mm.long()]) if with_boundary else base + me[mm.long()]
        assert torch.equal(got, ref), (rows, E)


# ---- heads and decoding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 252, 256, 260, 768, 1028])
def test_linear_heads(dev, lib, D):
    """logits[h][r] = <x[r], w_h> + b_h for 1, 2 and 3 heads (the unused weight pointers NULL) against fp64.  A lane adds its four
    products of every 256-wide column step in a chain (4 ceil(D / 256) serial roundings), the wave adds 64 lanes in 6 butterfly
    levels, then the bias: depth n = 4 ceil(D / 256) + 7, bar n U (sum |x w| + |b|).  Rows 1, 3, 4, 5, 1500, 9601 (tails of the
    4-row block); exactly nheads * rows outputs written."""
    depth = 4 * ((D + 255) // 256) + 7
    for rows in (1, 3, 4, 5, 1500, 9601):
        x = _rand((rows, D), rows * 7 + D)
        ws = [_rand(D, rows * 7 + D + 1 + h, std=0.2) for h in range(3)]
        b3 = _rand(3, rows + D, std=0.5)
        xd, w0, w1, w2, bd = _dev(dev, x, *ws, b3)
        wd = [w0, w1, w2]
        for nh in (1, 2, 3):
            lg = _out(dev, 3 * rows)
            _ok(lib.hirest_linear_heads(_p(xd), rows, D, nh, _p(wd[0]), _p(wd[1]) if nh > 1 else None, _p(wd[2]) if nh > 2 else None,
                                        _p(bd), _p(lg), _s()), "linear_heads")
            got = _body(lg, nh * rows, what=f"linear_heads rows={rows} D={D} nheads={nh}").double().view(nh, rows)
            W = torch.stack([w.double() for w in ws[:nh]])
            ref = W @ x.double().t() + b3.double()[:nh, None]
            bar = depth * U * (W.abs() @ x.double().abs().t() + b3.double().abs()[:nh, None]) + 1e-300
            _within((got - ref).abs(), bar, f"linear_heads rows={rows} D={D} nheads={nh}")


def _argmax_rows(T, fill, seed):
    """Rows of (logits, mask) for masked_argmax at width T: random; exact ties at (t, t + d) for d = 1 (neighbouring lanes), 64
    (neighbouring waves), 256 (one thread's stride), at the front, across the lane-63 / lane-0 and thread-255 / thread-0 seams and
    ending at T - 1 (there the lower index sits in a later wave); the maximum at 0 and at T - 1; all masked; unmasked logits equal
    to fill and below it; -inf logits, also everywhere."""
    g = torch.Generator().manual_seed(seed)
    xs, ms = [], []

    def base(p_on=0.7):
        return torch.randn(T, generator=g) * 3, (torch.rand(T, generator=g) < p_on).to(torch.int32)

    def add(x, m):
        xs.append(x)
        ms.append(m)
    add(*base())
    pairs = [(3, 1), (3, 64), (3, 256), (63, 1), (255, 1), (190, 64)] + [(T - 1 - d, d) for d in (1, 64, 256)]
    for a, d in pairs:
        if 0 <= a and a + d < T:
            x, m = base()
            top = x.abs().max() + 1.0
            x[a] = x[a + d] = top
            m[a] = m[a + d] = 1
            add(x, m)
    for at in (0, T - 1):
        x, m = base()
        x[at] = x.abs().max() + 1.0
        m[at] = 1
        add(x, m)
    x, _ = base()
    add(x, torch.zeros(T, dtype=torch.int32))                                     # all masked: fill everywhere -> 0
    x, m = base(0.9)
    x = fill - (1.0 + x.abs()) * (abs(fill) * 1e-3 + 1.0)                        # unmasked logits below fill (-inf stays -inf)
    add(x.clone(), m)
    x[min(T - 1, 7)] = fill                                                       # ... and one equal to it
    m[min(T - 1, 7)] = 1
    add(x, m)
    x, m = base()
    x[::3] = float("-inf")
    add(x, m)
    add(torch.full((T,), float("-inf")), torch.ones(T, dtype=torch.int32))       # -inf everywhere, unmasked
    x = torch.full((T,), float("-inf"))
    m = torch.ones(T, dtype=torch.int32)
    m[T // 2] = 0
    add(x, m)
    return torch.stack(xs).float(), torch.stack(ms)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 1855, 4097])
def test_masked_argmax_first_maximum(dev, lib, T):
    """out[b] = logits.masked_fill(mask == 0, fill).argmax(1) EXACTLY (torch: the first maximal index), fill = -1e10 (the model's)
    and -inf, over the rows of _argmax_rows.  B outputs written, nothing behind them."""
    for fill in (-1e10, float("-inf")):
        x, m = _argmax_rows(T, float(np.float32(fill)), T)
        B = x.shape[0]
        xd, md = _dev(dev, x, m)
        out = _out(dev, B, -7, torch.int32)
        _ok(lib.hirest_masked_argmax(_p(xd), _p(md), fill, B, T, _p(out), _s()), "masked_argmax")
        got = _body(out, B, -7, what="masked_argmax").long()
        ref = x.masked_fill(m == 0, float(np.float32(fill))).argmax(1)
        assert torch.equal(got, ref), f"T={T} fill={fill}: rows {(got != ref).nonzero().flatten().tolist()} got {got.tolist()} want {ref.tolist()}"


# ---- moment segmentation ------------------------------------------------------------------------------------------------------------
class _SegState:
    """moment_mask, boundary_mask, steps, nsteps of B samples on the device (with sentinels behind each) and as the reference's
    loop body (modeling.py:393-433) leaves them, given the kernel's own probabilities."""

    def __init__(self, dev, mm, bm, max_steps, nsteps=None):
        self.B, self.T = mm.shape
        self.max_steps = max_steps
        self.mm, self.bm = mm.clone(), bm.clone()
        self.steps = torch.full((self.B, max_steps, 2), -7, dtype=torch.int32)
        self.n = torch.zeros(self.B, dtype=torch.int32) if nsteps is None else nsteps.clone()
        self.d_mm, self.d_bm = _out(dev, mm.numel(), -5, torch.int32), _out(dev, mm.numel(), -5, torch.int32)
        self.d_mm[:mm.numel()] = mm.flatten().to(dev)
        self.d_bm[:mm.numel()] = bm.flatten().to(dev)
        self.d_steps = _out(dev, self.steps.numel(), -7, torch.int32)
        self.d_n = _out(dev, self.B, -5, torch.int32)
        self.d_n[:self.B] = self.n.to(dev)

    def launch(self, lib, dev, logits, thr):
        B, T = self.B, self.T
        ld, = _dev(dev, logits)
        probs = _out(dev, B * T)
        _ok(lib.hirest_segmentation_step(_p(ld), _p(self.d_mm), _p(self.d_bm), B, T, thr, _p(self.d_steps), _p(self.d_n), self.max_steps,
                                         _p(probs), _s()), "segmentation_step")
        return _body(probs, B * T, what="probs_out").view(B, T)

    def advance_reference(self, probs, thr):
        from oracle.ref_cpu import segmentation_walk
        walks = []
        for b in range(self.B):
            p = probs[b].tolist()
            w = segmentation_walk(p, int(np.argmax(probs[b].numpy())), thr)
            walks.append(w)
            if w is None:
                continue
            l, r = w
            self.mm[b, l:r + 1] = 0
            self.bm[b, l] = self.bm[b, r] = 1
            if self.n[b] < self.max_steps:
                self.steps[b, self.n[b]] = torch.tensor([l, r], dtype=torch.int32)
                self.n[b] += 1
        return walks

    def compare(self, what):
        n = self.B * self.T
        assert torch.equal(_body(self.d_mm, n, -5, what).view(self.B, self.T), self.mm), f"{what}: moment_mask"
        assert torch.equal(_body(self.d_bm, n, -5, what).view(self.B, self.T), self.bm), f"{what}: boundary_mask"
        assert torch.equal(_body(self.d_n, self.B, -5, what), self.n), f"{what}: nsteps"
        assert torch.equal(_body(self.d_steps, self.steps.numel(), -7, what).view(self.steps.shape), self.steps), f"{what}: steps"


def _seg_probs_check(probs, logits, mm, what):
    """probs_out against the fp64 softmax of logits.masked_fill(mask == 0, -finfo.max) (modeling.py:404-405).  Per probability:
    the exponent x - max carries two roundings (the difference, and its product by log2(e) inside expf): 2 U |x - max|; expf's own
    error (2 U); the row sum (ceil(T / 256) serial terms per thread, 6 butterfly levels, 2 more: (ceil(T / 256) + 8) U relative,
    shared by the row) and the quotient (U); doubled for the exp errors inside the sum:
    bar p U (2 |x - max| + ceil(T / 256) + 16) + 2^-126."""
    T = logits.shape[1]
    x = logits.double().masked_fill(mm == 0, -FMAX)
    ref = torch.softmax(x, 1)
    d = (x - x.amax(1, keepdim=True)).abs().clamp_max(1e3)            # (masked entries are exactly 0 in both)
    bar = ref * U * (2 * d + (T + 255) // 256 + 16) + 2.0 ** -126
    _within((probs.double() - ref).abs(), bar, what)


def _seg_logits(B, T, seed, peaks=None, width=None):
    """Noise plus a bump at a random (or given) frame per row: walks of every length."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T), generator=g, dtype=torch.float64)
    t = torch.arange(T, dtype=torch.float64)
    for b in range(B):
        c = int(torch.randint(0, T, (1,), generator=g)) if peaks is None or peaks[b] is None else peaks[b]
        w = width or max(1.0, T / float(torch.randint(4, 40, (1,), generator=g)))
        x[b] += 8.0 * torch.exp(-((t - c) / w) ** 2)
    return x.float()


@pytest.mark.parametrize("T", [1, 255, 256, 257, 300, 16384])
def test_segmentation_step_edges(dev, lib, T):
    """One step per threshold (0.5, 0.2, 0 and 1, 1.5) over rows that reach each edge: a peak at frame 0 (skipped: left bound 0),
    a peak at T - 1 (the right walk stops at the end), a mask ending at T - 1 (threshold 0 walks to it), a mask starting at 0 (walks
    to 0: skipped), an all-masked row (uniform 1 / T, argmax 0: skipped), a random span.  probs_out against fp64; given the first
    maximum of the kernel's OWN probabilities, oracle.ref_cpu.segmentation_walk on them as Python floats fixes moment_mask,
    boundary_mask, steps and nsteps EXACTLY.  T = 16384 is the largest T accepted (its probabilities fill 64 KiB of LDS).
    (With T <= 16384 the peak probability is at least 1 / T > 1e-5, so the reference's max_score < 1e-5 branch cannot be reached
    from any input: it is not tested.)"""
    B = 6
    for i, thr in enumerate((0.5, 0.2, 0.0, 1.0, 1.5)):
        peaks = [0, T - 1, None, None, None, None]
        x = _seg_logits(B, T, T + i, peaks)
        mm = torch.ones((B, T), dtype=torch.int32)
        bm = torch.zeros((B, T), dtype=torch.int32)
        lo, hi = T // 3, 2 * T // 3
        mm[2, :lo] = 0                                    # mask [lo, T - 1]
        mm[3, hi + 1:] = 0                                # mask [0, hi]
        mm[4] = 0                                         # all masked
        mm[5, :T // 5] = 0
        mm[5, T - T // 5:] = 0
        x[0, 0] += 20.0                                   # the maximum exactly at 0 ...
        x[1, T - 1] += 20.0                               # ... and at T - 1
        if T > 1:
            x[2, T - 1] += 3.0
            x[3, 0] += 3.0
        bm[:, T // 5] = 1
        s = _SegState(dev, mm, bm, max_steps=4)
        probs = s.launch(lib, dev, x, thr)
        _seg_probs_check(probs, x, mm, f"segmentation probs T={T} thr={thr}")
        walks = s.advance_reference(probs, thr)
        s.compare(f"segmentation T={T} thr={thr}")
        if T > 1 and thr == 0.0:
            assert walks[2] is not None and walks[2][1] == T - 1, walks        # reaches the right end
        if T > 1:
            assert walks[0] is None and walks[4] is None                        # peak at 0 / all masked: skipped


def test_segmentation_step_twenty_chained_calls(dev, lib):
    """The segmentation loop: 20 calls on one state (new logits each call, as the model's forward gives), B = 5, T = 300, masks
    carried over; after every call the state equals the oracle loop driven by the kernel's probabilities.  max_steps = 6, so
    the step lists fill up mid-way: later accepted walks still clear the mask and set the boundaries, but append nothing."""
    B, T = 5, 300
    g = torch.Generator().manual_seed(5)
    mm = torch.zeros((B, T), dtype=torch.int32)
    bm = torch.zeros((B, T), dtype=torch.int32)
    for b in range(B):
        a = int(torch.randint(1, 100, (1,), generator=g))
        e = int(torch.randint(200, T, (1,), generator=g))
        mm[b, a:e + 1] = 1
        bm[b, a] = 1
    s = _SegState(dev, mm, bm, max_steps=6)
    accepted = 0
    for it in range(20):
        x = _seg_logits(B, T, 1000 + it, width=6.0)
        probs = s.launch(lib, dev, x, 0.5)
        _seg_probs_check(probs, x, s.mm, f"chained probs it={it}")
        accepted += sum(w is not None for w in s.advance_reference(probs, 0.5))
        s.compare(f"chained it={it}")
    assert accepted > B * 6 and (s.n == 6).any(), (accepted, s.n.tolist())          # the lists did fill up


def test_segmentation_step_full_step_list(dev, lib):
    """nsteps == max_steps on entry: an accepted walk still clears moment_mask [l, r] and sets boundary_mask at l and r, and
    neither steps nor nsteps change."""
    B, T = 3, 257
    x = _seg_logits(B, T, 77, peaks=[100, 200, 50], width=5.0)
    mm = torch.ones((B, T), dtype=torch.int32)
    bm = torch.zeros((B, T), dtype=torch.int32)
    s = _SegState(dev, mm, bm, max_steps=3, nsteps=torch.full((B,), 3, dtype=torch.int32))
    probs = s.launch(lib, dev, x, 0.5)
    walks = s.advance_reference(probs, 0.5)
    assert all(w is not None for w in walks), walks
    s.compare("full step list")
    assert (s.mm == 0).any(1).all() and torch.equal(s.n, torch.full((B,), 3, dtype=torch.int32))


# ---- fp32 attention family -------------------------------------------------------------------------------------------------------
def _attn64(q, k, v, scale, addc, causal):
    """q [G, Tq, dh], k / v [G, Tk, dh] (fp32) -> fp64 context and its bar.  Per score: the kernel's dh-term fp32 dot product
    (dh U scale sum |q k|) and the one rounding of fl(qk scale + add_const) (U |S|: half an ulp of the shifted score — at
    add_const = -10000 this quantisation dominates, as in the reference's own fp32 scores); __expf of s - max adds U (|s - max| + 2).
    A probability moves by at most twice the largest of these (numerator and row sum); the P V chain and the row sum add (3 Tk + 16) U
    of sum p |v|.  Keys past a query (causal) are at -inf here: the kernel's penalty of -10000 or -1e30 must vanish in the exp."""
    q, k, v = q.double(), k.double(), v.double()
    S = q @ k.transpose(-1, -2) * scale + addc
    Tq, Tk = S.shape[-2:]
    masked = torch.zeros((Tq, Tk), dtype=torch.bool)
    if causal:
        masked = torch.arange(Tk)[None, :] > torch.arange(Tq)[:, None]
    S = S.masked_fill(masked, float("-inf"))
    P = torch.softmax(S, -1)
    m = S.amax(-1, keepdim=True)
    es = q.shape[-1] * U * scale * (q.abs() @ k.abs().transpose(-1, -2)) + U * S.abs() + U * ((S - m).abs() + 2)
    E = es.masked_fill(masked, 0.0).amax(-1, keepdim=True)
    return P @ v, (2 * E + (3 * Tk + 16) * U) * (P @ v.abs()) + 1e-300


def _heads(x, B, T, H, dh):
    return x.reshape(B, T, H, dh).permute(0, 2, 1, 3).reshape(B * H, T, dh)


# (B, Tq, Tk): Tq != Tk both ways; Tq = 64 runs one-wave blocks, 65 and 257 three-wave blocks, 128 and 300 four-wave blocks
ATTN_SHAPES = [(2, 1, 20), (1, 17, 300), (1, 300, 17), (2, 64, 64), (1, 65, 65), (1, 257, 257), (2, 128, 128), (1, 300, 300)]


@pytest.mark.parametrize("causal", [0.0, -10000.0, -1e30])
@pytest.mark.parametrize("dh", [20, 32, 64, 68, 88, 96])
def test_attention_f32_qkv(dev, lib, dh, causal):
    """hirest_attention_f32_qkv against fp64 (_attn64's bar) for head widths of all three instantiations (88: the fp32 vision
    tower), causal_penalty 0 / -10000 / -1e30 with keys j > i masked (top-left aligned, the diagonal visible), Tq != Tk, q / kv
    row strides wider than the packed width (NaN between: never read), add_const 0 and -10000.  Every output row is written and
    nothing behind the last one."""
    H = 2
    D = H * dh
    ldq, ldkv = D + 8, 2 * D + 12
    scale = float(np.float32(dh ** -0.5))
    for B, Tq, Tk in ATTN_SHAPES:
        for addc in (0.0, -10000.0):
            seed = dh * 100000 + Tq * 1000 + Tk + int(addc == 0.0)
            qb = torch.full((B * Tq, ldq), float("nan"))
            kvb = torch.full((B * Tk, ldkv), float("nan"))
            qb[:, :D] = _rand((B * Tq, D), seed)
            kvb[:, :2 * D] = _rand((B * Tk, 2 * D), seed + 1)
            qd, kvd = _dev(dev, qb, kvb)
            out = _out(dev, B * Tq * D)
            _ok(lib.hirest_attention_f32_qkv(_p(qd), ldq, _p(kvd), _p(kvd, D), ldkv, _p(out), B, Tq, Tk, H, dh, scale, addc, causal,
                                             _s()), "attention_f32_qkv")
            what = f"attention_f32_qkv dh={dh} causal={causal:g} B={B} Tq={Tq} Tk={Tk} add={addc:g}"
            got = _heads(_body(out, B * Tq * D, what=what), B, Tq, H, dh)
            ref, bar = _attn64(_heads(qb[:, :D], B, Tq, H, dh), _heads(kvb[:, :D], B, Tk, H, dh), _heads(kvb[:, D:2 * D], B, Tk, H, dh),
                               scale, addc, causal != 0.0)
            _within((got.double() - ref).abs(), bar, what)


@pytest.mark.parametrize("dh", [32, 64])
def test_attention_f32_varlen(dev, lib, dh):
    """One call over ragged sequences against per-sequence fp64 (_attn64): lengths 1, 2, 31, 32, 33, 64, 65, 129, 300 and a
    zero-length one, across the 32-query wave and the 64 / 96 / 128-query blocks (four-wave form, max_len 300); then lengths up
    to 64 (one-wave form).  Every row of the packed output is written, nothing behind it."""
    H = 3
    D = H * dh
    scale = float(np.float32(dh ** -0.5))
    for lens in ([1, 2, 31, 0, 32, 33, 64, 65, 129, 300], [1, 2, 0, 31, 32, 33, 64]):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        n = int(off[-1])
        qkv = _rand((n, 3 * D), dh * 1000 + len(lens))
        qd, od = _dev(dev, qkv, torch.from_numpy(off))
        out = _out(dev, n * D)
        _ok(lib.hirest_attention_f32_varlen(_p(qd), _p(out), _p(od), len(lens), max(lens), H, dh, scale, 0.0, _s()), "varlen")
        got = _body(out, n * D, what="varlen").view(n, D)
        for i, L in enumerate(lens):
            if L == 0:
                continue
            rows = qkv[off[i]:off[i + 1]]
            ref, bar = _attn64(_heads(rows[:, :D], 1, L, H, dh), _heads(rows[:, D:2 * D], 1, L, H, dh), _heads(rows[:, 2 * D:], 1, L, H, dh),
                               scale, 0.0, False)
            _within((_heads(got[off[i]:off[i + 1]], 1, L, H, dh).double() - ref).abs(), bar, f"varlen dh={dh} len={L} max_len={max(lens)}")


@pytest.mark.parametrize("t_hist", [0, 1, 31, 32, 47])
def test_attention_f32_decode_self(dev, lib, t_hist):
    """A decoding step's self-attention: row r attends over the history of its parent row (parent non-identity, with repeats) plus
    its own newest key, against fp64 (_attn64's bar); k_out / v_out receive exactly the gathered history with the new key appended.
    The context and both histories written in full, nothing behind them."""
    R, H = 6, 2
    D = H * 64
    T = t_hist + 1
    qkv = _rand((R, 3 * D), 50 + t_hist, std=1.5)
    kh, vh = _rand((R, max(t_hist, 1), D), 60 + t_hist, std=1.5), _rand((R, max(t_hist, 1), D), 70 + t_hist, std=1.5)
    parent = torch.tensor([2, 2, 0, 5, 1, 3], dtype=torch.int32)
    qd, khd, vhd, pd = _dev(dev, qkv, kh, vh, parent)
    out, ko, vo = _out(dev, R * D), _out(dev, R * T * D), _out(dev, R * T * D)
    _ok(lib.hirest_attention_f32_decode(_p(qd), 3 * D, _p(khd) if t_hist else None, _p(vhd) if t_hist else None, D, _p(pd) if t_hist else None,
                                        t_hist, _p(qd, D), _p(qd, 2 * D), 3 * D, _p(ko), _p(vo), _p(out), R, H, 0.125, 0.0, 0.0, _s()), "decode")
    src = parent.long() if t_hist else torch.arange(R)
    kc = torch.cat([kh[src][:, :t_hist], qkv[:, None, D:2 * D]], 1)
    vc = torch.cat([vh[src][:, :t_hist], qkv[:, None, 2 * D:]], 1)
    assert torch.equal(_body(ko, R * T * D, what="k_out").view(R, T, D), kc)
    assert torch.equal(_body(vo, R * T * D, what="v_out").view(R, T, D), vc)
    got = _body(out, R * D, what="decode out").view(R, H, 1, 64)
    q = qkv[:, :D].reshape(R, H, 1, 64)
    k, v = kc.reshape(R, T, H, 64).transpose(1, 2), vc.reshape(R, T, H, 64).transpose(1, 2)
    ref, bar = _attn64(q, k, v, 0.125, 0.0, False)
    _within((got.double() - ref).abs(), bar, f"decode self t_hist={t_hist}")


def test_attention_f32_decode_cross(dev, lib):
    """The decoder's cross-attention: one query per row over its F = 20 encoded frames ([R, F, 2 D] key | value rows, no parent,
    no new key), add_const -10000 as caption.hip passes it, against fp64 (_attn64's bar)."""
    R, H, F = 7, 3, 20
    D = H * 64
    q, enc = _rand((R, D), 81), _rand((R, F, 2 * D), 82)
    qd, ed = _dev(dev, q, enc)
    out = _out(dev, R * D)
    _ok(lib.hirest_attention_f32_decode(_p(qd), D, _p(ed), _p(ed, D), 2 * D, None, F, None, None, 0, None, None, _p(out), R, H, 0.125,
                                        -10000.0, 0.0, _s()), "decode cross")
    got = _body(out, R * D, what="decode cross").view(R, H, 1, 64)
    k, v = enc[..., :D].reshape(R, F, H, 64).transpose(1, 2), enc[..., D:].reshape(R, F, H, 64).transpose(1, 2)
    ref, bar = _attn64(q.reshape(R, H, 1, 64), k, v, 0.125, -10000.0, False)
    _within((got.double() - ref).abs(), bar, "decode cross F=20")


# ---- beam search against the reference's Beam ---------------------------------------------------------------------------------------
def _beam_logits(g, B, beam, V, step, eos, sep_mid):
    """Synthetic logits of one step: sample 0 emits [SEP] at step 0 (its beam-0 row), sample 1 at step sep_mid (every beam), the
    others never ([SEP] far below the rest)."""
    x = torch.randn((B * beam, V), generator=g) * 3.0
    x[:, eos] = -30.0
    if step == 0:
        x[0, eos] = x[0].max() + 20.0
    if step == sep_mid:
        x[beam:2 * beam, eos] = x[beam:2 * beam].max() + 20.0
    return x


@pytest.mark.parametrize("beam", [1, 3, 5, 16])
@pytest.mark.parametrize("fused", [True, False], ids=["tail", "separate"])
def test_beam_search_equals_reference_beam(dev, lib, beam, fused):
    """A whole beam search over B = 4 samples and 12 steps, step by step against oracle.ref_cpu.RefBeam (beam.py), through the fused
    tail (hirest_caption_beam_tail) or the separate kernels (hirest_log_softmax_f32 + hirest_topk_f32_ws + hirest_beam_advance, the
    caption_fused_tail = False path).  RefBeam advances on the kernel's own log-probabilities (hirest_log_softmax_f32, row_add 0):
    its fp32 score adds are then the kernel's, so tokens, back-pointers, scores, done flags and step counts must match EXACTLY after
    every step, and the next step's ids / parents / row_add with them.  Step 0 uses the model's convention (row_add -3e38 on beams
    > 0) against RefBeam reading row 0 only.  Then hirest_beam_backtrack against RefBeam.hypothesis of the best beam.  The synthetic
    logits carry no exact tie among a sample's top beam + 1 candidates (asserted): the tie order is covered elsewhere."""
    from oracle.ref_cpu import RefBeam, EOS_ID
    B, V, max_steps, sep_mid = 4, 5000, 12, 5
    R = B * beam
    st = _s()
    g = torch.Generator().manual_seed(beam)
    refs = [RefBeam(beam) for _ in range(B)]
    i32 = dict(dtype=torch.int32, device=dev)
    scores = torch.zeros(R, device=dev)
    tokens = torch.full((B, max_steps, beam), -7, **i32)
    backptr = torch.full((B, max_steps, beam), -7, **i32)
    n_steps, done = torch.zeros(B, **i32), torch.zeros(B, **i32)
    ids, parents, nadd = torch.full((R,), -7, **i32), torch.full((R,), -7, **i32), torch.full((R,), float("nan"), device=dev)
    add = torch.full((B, beam), -3.0e38)
    add[:, 0] = 0.0
    add = add.reshape(-1).to(dev)
    logp = torch.empty((R, V), device=dev)
    logp2 = torch.empty((R, V), device=dev)
    tws = torch.empty(max(int(lib.hirest_caption_beam_tail_workspace_bytes(B, beam, V)), 16), dtype=torch.uint8, device=dev)
    kws = torch.empty(max(int(lib.hirest_topk_workspace_bytes(B, beam * V, beam)), 16), dtype=torch.uint8, device=dev)
    val, idx = torch.empty((B, beam), device=dev), torch.empty((B, beam), **i32)
    exp_tok = torch.full((B, max_steps, beam), -7, dtype=torch.int32)
    exp_bp = torch.full((B, max_steps, beam), -7, dtype=torch.int32)
    for step in range(max_steps):
        x = _beam_logits(g, B, beam, V, step, EOS_ID, sep_mid)
        xd = x.to(dev)
        _ok(lib.hirest_log_softmax_f32(_p(xd), V, None, _p(logp), V, R, V, st), "log_softmax")
        lp = logp.cpu()
        was_done = [r.done for r in refs]
        for b in range(B):
            if was_done[b]:
                continue
            lpb = lp[b * beam:(b + 1) * beam]
            lk = (lpb + refs[b].scores.unsqueeze(1) if refs[b].prev_ks else lpb[0]).reshape(-1)
            top = lk.topk(min(beam + 1, lk.numel())).values
            assert bool((top[1:] < top[:-1]).all()), f"step {step} sample {b}: a tie in the synthetic data"
            refs[b].advance(lpb)
            exp_tok[b, step] = torch.tensor(refs[b].next_ys[-1], dtype=torch.int32)
            exp_bp[b, step] = torch.tensor(refs[b].prev_ks[-1], dtype=torch.int32)
        if fused:
            _ok(lib.hirest_caption_beam_tail(_p(xd), V, _p(add), B, beam, V, step, max_steps, EOS_ID, _p(scores), _p(tokens), _p(backptr),
                                             _p(n_steps), _p(done), _p(ids), _p(parents), _p(nadd), None, _p(tws), tws.numel(), st), "tail")
        else:
            _ok(lib.hirest_log_softmax_f32(_p(xd), V, _p(add), _p(logp2), V, R, V, st), "log_softmax + row_add")
            _ok(lib.hirest_topk_f32_ws(_p(logp2), None, B, beam * V, beam, _p(idx), _p(val), _p(kws), kws.numel(), st), "topk")
            _ok(lib.hirest_beam_advance(_p(val), _p(idx), B, beam, V, step, max_steps, EOS_ID, _p(scores), _p(tokens), _p(backptr),
                                        _p(n_steps), _p(done), _p(ids), _p(parents), _p(nadd), st), "beam_advance")
        what = f"beam={beam} {'tail' if fused else 'separate'} step {step}"
        assert torch.equal(tokens.cpu(), exp_tok), f"{what}: tokens"
        assert torch.equal(backptr.cpu(), exp_bp), f"{what}: backptr"
        assert torch.equal(scores.cpu().view(B, beam), torch.stack([r.scores for r in refs])), f"{what}: scores"
        assert done.cpu().tolist() == [int(r.done) for r in refs], f"{what}: done"
        assert n_steps.cpu().tolist() == [len(r.prev_ks) for r in refs], f"{what}: n_steps"
        want_ids, want_par, want_add = [], [], []
        for b in range(B):
            for k in range(beam):
                if was_done[b]:
                    want_ids.append(EOS_ID); want_par.append(b * beam + k); want_add.append(0.0)
                else:
                    want_ids.append(refs[b].next_ys[-1][k]); want_par.append(b * beam + refs[b].prev_ks[-1][k])
                    want_add.append(refs[b].scores[k].item())
        assert ids.cpu().tolist() == want_ids and parents.cpu().tolist() == want_par, f"{what}: next ids / parents"
        assert torch.equal(nadd.cpu(), torch.tensor(want_add, dtype=torch.float32)), f"{what}: next row_add"
        add = nadd.clone()
    assert [r.done for r in refs] == [True, True, False, False] and [len(r.prev_ks) for r in refs] == [1, sep_mid + 1, max_steps, max_steps]
    out = _out(dev, B * (max_steps + 1), -7, torch.int32)
    _ok(lib.hirest_beam_backtrack(_p(scores), _p(tokens), _p(backptr), _p(n_steps), B, beam, max_steps, _p(out), st), "backtrack")
    got = _body(out, B * (max_steps + 1), -7, what="backtrack").view(B, max_steps + 1)
    for b in range(B):
        k = int(torch.sort(refs[b].scores, 0, True)[1][0])
        hyp = refs[b].hypothesis(k)
        want = [len(hyp)] + hyp + [-7] * (max_steps - len(hyp))
        assert got[b].tolist() == want, (b, got[b].tolist(), want)
    assert got[0, :2].tolist() == [1, EOS_ID] and got[1, sep_mid + 1].item() == EOS_ID
