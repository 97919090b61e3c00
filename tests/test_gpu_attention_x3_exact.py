"""The split-operand attention (csrc/attention_x3.hip: hirest_attention_x3_qkv and hirest_attention_x3_qkv_split2, the attention of the
bf16x3 vision tower and of the bf16x3 Whisper encoder) per element, at the shapes where its tiling changes: one key tile, two, the first
fetch at k0 + 64 and the steady state of the double buffer, ragged last tiles, one to ten waves of queries, Tq != Tk, head widths 4 (the
dh - 4 clamp is 0), 36 and 68 (four columns into the next padded width), 88 and 96.

Five input families (tests/_exact_inputs.py; their preconditions are checked in tests/test_exact_inputs_host.py):
  1. x3_selector_klo / x3_selector_qlo: one key takes the whole softmax and the selection rides on q_hi k_lo (or q_lo k_hi) alone; the
     output row must be that key's V row bit for bit, and V needs both of its parts;
  2. x3_uniform: q = 0 and an indicator V, the output is a count of keys over their number;
  3. x3_isolation: the neighbouring frame and what lies after the operands would dominate or overflow if ever read as keys;
  4. x3_random, with the error per element relative to the column's own maximum, measured against the fp64 restatement of the operand
     format (never against the kernel).

Every call runs with the operands packed ([B * T, 3 D] rows, only where Tq == Tk) and separate: q in one allocation with ldq = D + 4, k | v in
a second with ldkv = 2 D + 8, NaN in the gap columns, TAIL_ROWS rows of NaN (q, v) and 3e38 (k) after each operand inside its allocation,
and the outputs inside sentinel-filled buffers whose GUARD_ROWS rows before and after must keep their bits."""
import pytest
import torch

import _exact_inputs as X

pytestmark = pytest.mark.gpu

SENT32, SENT16 = 0x5A5B5C5D, 0x5A5B            # as fp32 1.5e16, as bf16 1.5e16: no output of any family
GUARD_ROWS = 8
TAIL_ROWS = 32
BADARG, SHAPE = -1, -2
WAVES = (0, 3, 4, 8, 9)

ALL = X.x3a_cases()
SEL = X.x3a_cases([dh for dh in X.X3A_DH if dh >= 32])
cases = lambda c: pytest.mark.parametrize("B,Tq,Tk,H,dh", c, ids=[X.x3a_id(x) for x in c])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class Operands:
    """q, k, v [B, T, H, dh] fp32 on the device in one of the two layouts; .q / .k / .v are byte addresses, .ldq / .ldkv row strides in
    floats.  frame(b) is the same memory addressed as a one-frame call."""

    def __init__(self, q, k, v, layout, dev, poison=True):
        B, Tq, H, dh = q.shape
        Tk, D = k.shape[1], H * dh
        self.dims, self.D = (B, Tq, Tk, H, dh), D
        tail = TAIL_ROWS if poison else 0
        if layout == "packed":
            assert Tq == Tk
            buf = torch.empty((B * Tq + tail, 3 * D), dtype=torch.float32, device=dev)
            buf[:B * Tq] = torch.cat([t.reshape(B * Tq, D) for t in (q, k, v)], dim=1).to(dev)
            buf[B * Tq:] = float("nan")
            buf[B * Tq:, D:2 * D] = 3e38
            self.keep = (buf,)
            self.q, self.k, self.v = buf.data_ptr(), buf.data_ptr() + 4 * D, buf.data_ptr() + 8 * D
            self.ldq = self.ldkv = 3 * D
        else:
            qb = torch.full((B * Tq + tail, D + 4), float("nan"), dtype=torch.float32, device=dev)
            qb[:B * Tq, :D] = q.reshape(B * Tq, D).to(dev)
            kv = torch.full((B * Tk + tail, 2 * D + 8), float("nan"), dtype=torch.float32, device=dev)
            kv[:B * Tk, :D] = k.reshape(B * Tk, D).to(dev)
            kv[:B * Tk, D + 4:2 * D + 4] = v.reshape(B * Tk, D).to(dev)
            kv[B * Tk:, :D] = 3e38
            self.keep = (qb, kv)
            self.q, self.k, self.v = qb.data_ptr(), kv.data_ptr(), kv.data_ptr() + 4 * (D + 4)
            self.ldq, self.ldkv = D + 4, 2 * D + 8

    def frame(self, b):
        B, Tq, Tk, H, dh = self.dims
        one = object.__new__(Operands)
        one.dims, one.D, one.keep, one.ldq, one.ldkv = (1, Tq, Tk, H, dh), self.D, self.keep, self.ldq, self.ldkv
        one.q = self.q + 4 * b * Tq * self.ldq
        one.k, one.v = self.k + 4 * b * Tk * self.ldkv, self.v + 4 * b * Tk * self.ldkv
        return one


def layouts(Tq, Tk):
    return ("packed", "separate") if Tq == Tk else ("separate",)


def _call(ops_, out_ptr, split2, scale=None):
    from hirest_amd import _lib, ops
    B, Tq, Tk, H, dh = ops_.dims
    fn = _lib.load().hirest_attention_x3_qkv_split2 if split2 else _lib.load().hirest_attention_x3_qkv
    return fn(ops_.q, ops_.ldq, ops_.k, ops_.v, ops_.ldkv, out_ptr, B, Tq, Tk, H, dh, dh ** -0.5 if scale is None else scale, ops.stream_ptr())


def run(ops_, dev, split2=False, waves=0):
    """One call into a sentinel-filled buffer with guard rows on both sides: [B, Tq, H, dh] fp32, or [B * Tq, 2 D] bf16 for the split2 entry.
    Every output element was written and no guard row was."""
    from hirest_amd import _lib
    B, Tq, Tk, H, dh = ops_.dims
    rows, D = B * Tq, ops_.D
    if split2:
        buf = torch.full((rows + 2 * GUARD_ROWS, 2 * D), SENT16, dtype=torch.int16, device=dev)
    else:
        buf = torch.full((rows + 2 * GUARD_ROWS, D), SENT32, dtype=torch.int32, device=dev)
    sent = SENT16 if split2 else SENT32
    lib = _lib.load()
    _lib.check(lib.hirest_attention_x3_select_waves(waves), "select_waves")
    try:
        _lib.check(_call(ops_, buf[GUARD_ROWS].data_ptr(), split2), "hirest_attention_x3_qkv" + ("_split2" if split2 else ""))
    finally:
        lib.hirest_attention_x3_select_waves(0)
    assert (buf[:GUARD_ROWS] == sent).all() and (buf[GUARD_ROWS + rows:] == sent).all(), "a guard row was written"
    body = buf[GUARD_ROWS:GUARD_ROWS + rows]
    assert not (body == sent).any(), "an output element was not written"
    return body.view(torch.bfloat16) if split2 else body.view(torch.float32).reshape(B, Tq, H, dh)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("family", ["klo", "qlo"])
@cases(SEL)
def test_selector_is_bit_exact(dev, B, Tq, Tk, H, dh, family):
    """Family 1: out[b, i, h] == v[b, pi(i), h] bit for bit, and the split2 output is split2_cpu of those rows, in both layouts, for the
    automatic geometry and forced 3, 4, 8 and 9 waves.  A wrong key, head, frame, row stride or batch offset, a dropped k_lo q_hi (klo) or
    k_hi q_lo (qlo) or v_lo p_hi term, a k-slot of P^T that meets the wrong key of V^T, or a mask that hides key pi(i) (key Tk - 1 and one
    key of every tile are always selected) gives another row."""
    d = (X.x3_selector_klo if family == "klo" else X.x3_selector_qlo)(B, Tq, Tk, H, dh)
    want = d["want"].to(dev)
    want2 = X.split2_cpu(d["want"].reshape(B * Tq, H * dh)).to(dev) if (H * dh) % 32 == 0 else None
    for layout in layouts(Tq, Tk):
        o = Operands(d["q"], d["k"], d["v"], layout, dev)
        for waves in WAVES:
            assert torch.equal(bits(run(o, dev, waves=waves)), bits(want)), (layout, waves)
            if want2 is not None:
                assert torch.equal(bits(run(o, dev, split2=True, waves=waves)), bits(want2)), (layout, waves)


@cases(ALL)
def test_uniform_counts_keys(dev, B, Tq, Tk, H, dh):
    """Family 2: |out - count_d / Tk| <= 2^-22 count_d / Tk per element (X.x3_uniform: two fp32 roundings of 2^-24 each, a factor 2 in
    hand; exactly 0 where no key has j % dh == d).  One key too many or too few is off by at least 1 / count of the value.
    Worst error / bound observed on the MI355X over the cases: 0.163 (Tk = 289, dh = 32; exactly 0 where Tk is a power of two)."""
    d = X.x3_uniform(B, Tq, Tk, H, dh)
    worst = 0.0
    for layout in layouts(Tq, Tk):
        o = Operands(d["q"], d["k"], d["v"], layout, dev)
        for waves in (0, 9):
            out = run(o, dev, waves=waves)
            err = (out.cpu().double() - d["ref"]).abs()
            assert (err <= d["bound"]).all(), (layout, waves, (err / d["bound"].clamp_min(1e-300)).max().item())
            worst = max(worst, (err[d["bound"] > 0] / d["bound"][d["bound"] > 0]).max().item())
            if (H * dh) % 32 == 0:
                assert torch.equal(bits(run(o, dev, split2=True, waves=waves)), bits(X.split2_cpu(out.cpu().reshape(B * Tq, H * dh)).to(dev))), (layout, waves)
    print(f"uniform {X.x3a_id((B, Tq, Tk, H, dh))}: worst error / bound {worst:.4f}")


@cases(ALL)
def test_isolation_from_neighbours_and_tail(dev, B, Tq, Tk, H, dh):
    """Family 3.  With NaN (q, v) and 3e38 (k) in the rows after each operand and a neighbouring frame whose keys would win by 400: the
    result is finite, within twice the restatement's own error of fp64 per element, bit-equal to the same call on allocations without the
    poisoned tail and to a second run; with B = 3, frame 1 and the last frame (the poison right behind it) are bit-equal to those frames
    run alone from the same memory: a frame's bits do not depend on the batch.  (The factor 2 is that of the random family's bar (a); the
    fp32 emulation comes to 0.95 - 1.05 of the restatement's error on these inputs, the kernel on the MI355X to 0.92 - 1.12.)"""
    d = X.x3_isolation(B, Tq, Tk, H, dh)
    q, k, v = d["q"], d["k"], d["v"]
    ref, cm = X.attention_x3_ref(q, k, v), X.x3_column_max(v)
    Y = ((X.attention_x3_restated(q, k, v) - ref).abs() / cm).max().item()
    for layout in layouts(Tq, Tk):
        o = Operands(q, k, v, layout, dev)
        out = run(o, dev)
        assert torch.isfinite(out).all(), layout
        e = ((out.cpu().double() - ref).abs() / cm).max().item()
        print(f"isolation {X.x3a_id((B, Tq, Tk, H, dh))} {layout}: worst error / column max {e:.2e}, restatement {Y:.2e}, ratio {e / Y:.2f}")
        assert e <= 2 * Y, (layout, e, Y)
        assert torch.equal(bits(out), bits(run(o, dev))), layout
        assert torch.equal(bits(out), bits(run(Operands(q, k, v, layout, dev, poison=False), dev))), layout
        for b in sorted({1, B - 1} if B > 1 else ()):
            for waves in (0, 9):
                assert torch.equal(bits(run(o.frame(b), dev, waves=waves)[0]), bits(out[b])), (layout, b, waves)
        if (H * dh) % 32 == 0:
            out2 = run(o, dev, split2=True)
            assert torch.equal(bits(out2), bits(X.split2_cpu(out.cpu().reshape(B * Tq, H * dh)).to(dev))), layout
            for b in sorted({1, B - 1} if B > 1 else ()):
                assert torch.equal(bits(run(o.frame(b), dev, split2=True)), bits(out2[b * Tq:(b + 1) * Tq])), (layout, b)


@pytest.mark.parametrize("qscale", [1, 3, 6])
@cases(ALL)
def test_random_inputs_per_element(dev, B, Tq, Tk, H, dh, qscale):
    """Family 4.  e[i, d] = |out - x| / colmax[d] with colmax the maximum of |v| over the keys of that frame, head and column (V column 1
    is 64 times larger and column 2 64 times smaller than the others, so every column is held to its own scale).
      (a) against the fp64 reference: worst e <= 2 Y, Y the worst e of X.attention_x3_restated, the fp64 statement of the operand format
          (hi lo + lo hi + hi hi for both products).  The margin: the fp32 emulation of the kernel comes to 0.90 - 1.09 of Y on the CPU.
      (b) against the restatement itself: worst e <= 4 E, E that of X.attention_x3_emulated (4, not 2: the emulation's fp32 summation
          order is not the MFMA's).  E is 3 to 10 times below Y, so (b) is the sharper bar.
    Both layouts; the split2 output is split2 of the fp32 output bit for bit.
    Whole-tensor, max |out - ref| / max |ref|, is printed next to the same restatement of bar (a), 2 Y max colmax / max |ref|.  That bar
    is looser than the 3e-5 of test_attention_x3_against_fp64 wherever colmax is far above |ref| (the softmax averages the x 64 column
    down) or Y itself is large (q scale 3 and 6: the lo x lo score term the format drops is 2^-16 of |q| |k| and passes through exp):
    it is a bar per element, each relative to its own column, and (b) holds the kernel far tighter than either.
    Observed on the MI355X (profiles/attention_x3_exact.txt): (a) 0.945 - 1.174 of Y, (b) at most 1.909 of E; whole-tensor 1.1e-6 - 3.3e-5,
    above 3e-5 in two cases at q scale 6 (B3-Tq289-Tk33-H3-dh4: 3.32e-5, B3-Tq64-Tk65-H2-dh32: 3.10e-5), where the kernel sits at 1.00 of Y:
    that is the operand format's own error at logits of that size, and the fp32 emulation on the CPU gives the same figures."""
    d = X.x3_random(B, Tq, Tk, H, dh, qscale)
    q, k, v = d["q"], d["k"], d["v"]
    ref, rst, cm = X.attention_x3_ref(q, k, v), X.attention_x3_restated(q, k, v), X.x3_column_max(v)
    Y = ((rst - ref).abs() / cm).max().item()
    E = ((X.attention_x3_emulated(q, k, v).double() - rst).abs() / cm).max().item()
    tag = f"random {X.x3a_id((B, Tq, Tk, H, dh))} qscale={qscale}"
    failed = []
    for layout in layouts(Tq, Tk):
        o = Operands(q, k, v, layout, dev)
        out = run(o, dev)
        got = out.cpu().double()
        a = ((got - ref).abs() / cm).max().item()
        b = ((got - rst).abs() / cm).max().item()
        whole = (got - ref).abs().max().item() / ref.abs().max().item()
        whole_bar = 2 * Y * cm.max().item() / ref.abs().max().item()
        ra, rb = a / Y if Y else a, b / E if E else b                # (one key: p = 1 and E = 0, the kernel must meet the restatement exactly)
        print(f"{tag} {layout}: Y {Y:.2e} (a) {ra:.3f} of Y | E {E:.2e} (b) {rb:.3f} of E | whole {whole:.2e} (bar (a) restated {whole_bar:.2e})")
        if not a <= 2 * Y:
            failed.append((layout, "a", ra))
        if not b <= 4 * E:
            failed.append((layout, "b", rb))
        if (H * dh) % 32 == 0:
            assert torch.equal(bits(run(o, dev, split2=True)), bits(X.split2_cpu(out.cpu().reshape(B * Tq, H * dh)).to(dev))), layout
    assert not failed, failed


def test_nine_wave_choice_keeps_the_bits(dev):
    """Tq = Tk = 257 with B * H = 512 and dh = 32 is the one shape class where the entry picks nine-wave workgroups by itself (waves == 9 &&
    B * H >= 512): the automatic call is bit-equal to forced 4 and forced 9 waves.  The launch records of hirest_profile_collect carry no
    block size (and this entry writes none), so that the automatic call did take nine waves is not shown here: only the equality is."""
    B, T, H, dh = 64, 257, 8, 32
    g = torch.Generator().manual_seed(257)
    q, k, v = (torch.randn((B, T, H, dh), generator=g) for _ in range(3))
    o = Operands(q, k, v, "packed", dev)
    auto = run(o, dev)
    assert torch.isfinite(auto).all()
    for waves in (4, 9):
        assert torch.equal(bits(run(o, dev, waves=waves)), bits(auto)), waves
    # frame 37 alone takes three-wave workgroups (B * H = 8): same bits again
    assert torch.equal(bits(run(o.frame(37), dev)[0]), bits(auto[37]))


def test_refusals_leave_the_output_alone(dev):
    """Every refusal of the entry returns its code before a launch: the output buffer keeps its sentinel."""
    from hirest_amd import _lib
    lib = _lib.load()
    B, Tq, Tk, H, dh = 2, 33, 40, 2, 32
    D = H * dh
    z = lambda T: torch.zeros((B, T, H, dh))
    base = Operands(z(Tq), z(Tk), z(Tk), "separate", dev)
    out = torch.full((B * Tq + 1, D), SENT32, dtype=torch.int32, device=dev)
    out2 = torch.full((B * Tq + 1, 2 * D), SENT16, dtype=torch.int16, device=dev)

    def expect(code, what, split2=None, out_off=0, **change):
        o = base.frame(0)
        o.dims = base.dims
        for name, val in change.items():
            setattr(o, name, val)
        for s2 in ((False, True) if split2 is None else (split2,)):
            ptr = (out2 if s2 else out).data_ptr() + out_off
            assert _call(o, ptr, s2, scale=0.125) == code, (what, s2)
        torch.cuda.synchronize()
        assert (out == SENT32).all() and (out2 == SENT16).all(), what

    for bad in (0, 6, 100):
        expect(SHAPE, f"dh {bad}", dims=(B, Tq, Tk, H, bad))
    for off in (1, 2, 3):
        expect(SHAPE, f"ldq + {off}", ldq=base.ldq + off)
        expect(SHAPE, f"ldkv + {off}", ldkv=base.ldkv + off)
    for off in (4, 8):
        for name in ("q", "k", "v"):
            expect(SHAPE, f"{name} + {off} bytes", **{name: getattr(base, name) + off})
        expect(SHAPE, f"out + {off} bytes", split2=False, out_off=off)
    for off in (2, 4):
        expect(SHAPE, f"out2 + {off} bytes", split2=True, out_off=off)
    expect(SHAPE, "out2 with D % 32 != 0", split2=True, dims=(B, Tq, Tk, 2, 36))
    for i, name in ((0, "B"), (1, "Tq"), (2, "Tk"), (3, "H")):
        dims = list(base.dims)
        dims[i] = 0
        expect(BADARG, f"{name} = 0", dims=tuple(dims))
    for name in ("q", "k", "v"):
        expect(BADARG, f"{name} NULL", **{name: None})
    assert _call(base, None, False) == BADARG and _call(base, None, True) == BADARG
    assert lib.hirest_attention_x3_select_waves(5) == BADARG and lib.hirest_attention_x3_select_waves(-1) == BADARG
    # and the refused selection changed nothing: the same operands run
    assert torch.equal(bits(run(base, dev)), torch.zeros((B, Tq, H, dh), dtype=torch.int32, device=dev))
