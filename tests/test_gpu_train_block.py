"""hirest_train_block_forward / _backward (csrc/train_block.hip) as a whole against float64 autograd with dropout on: the nine kept
activations, dx and the sixteen parameter gradients, element by element, against tests/_train_ref.py (block_ref, checked on the CPU
in tests/test_train_block_ref_host.py) with the same dropout masks, at small shapes where tiles, waves and scratch slices end
(_train_ref.CASES), in both precisions.  The entry points are called through _lib.load() with _lib.TrainBlock / _lib.TrainBlockGrads
the way train._block_forward / _block_backward fill them, with a column-sum table and a side stream of the test's own.

Every buffer the block writes (activations, gradients, both scratches, both GEMM workspaces) lives in one arena, NaN-filled, with at
least 256 bytes of a bit pattern before and after it, and the scratch sizes are exactly what *_scratch_bytes() return: every run
checks that the pattern is intact and that no output element is still NaN.

Bars, per tensor, E = max |got - ref64|:
  precision 0   E <= 4 E_y + 2^-23 max|ref64|.  E_y: the error of block_ref in fp32 on the CPU with the same masks; 4: the project's
                bar for a chain of fp32 GEMMs against the CPU's fp32 evaluation (test_encoder_against_fp64); the
                additive term: two roundings of the largest element, for tensors where the yardstick happens to land within a
                rounding of fp64 (test_gpu_optim.py).
  precision 1   E <= E_bf / 50.  E_bf: the error of the "bf16 GEMM" yardstick (block_ref with the operands of the four forward and
                the four dX products rounded to bf16); 1 / 50: what test_gemm_x3_against_fp64 asserts per product.  Two tensors have
                E_bf = 0 exactly and keep the precision 0 bar instead (FP32_ONLY; the test asserts that they are the only ones): P,
                because the builder's scores are exact with bf16 operands too, and g_ln2_b, column sums of dout with no product in
                front of them.  Attention and the column sums run in fp32 kernels in both precisions.
  g_bqkv's key third is zero in exact arithmetic (each row of dS sums to zero), so the reference is rounding noise and so is E_y:
                E <= 4 E_y + 2^-23 max|g_bqkv ref64| in both precisions (the fp32 yardstick's floor only; E_bf is 1e-17 there).
In both precisions P is zero nowhere the reference is not, and a_pre - x, x_pre - aa are exactly zero where the restated masks drop
and non-zero where they keep (wherever the reference's update is above 2^-20 of the element it is added to).

Measured on an MI355X (worst over every case, drop and attention implementation; E / E_y and E / E_bf are printed per tensor):
  precision 0   E / bar 0.54 (g_ln2_g, case x3, drop 0.5); E / E_y at most 2.7.
  precision 1   E / bar 0.41 (g_b2, case x3, drop 0.1: E / E_bf = 0.0082 = 1 / 122), 0.09 - 0.21 for the other tensors behind a split-operand
                product; every one clears 1 / 50 by more than a factor 2, so 1 / 50 holds for all of them.  P: 0.31 and g_ln2_b: 0.28 of the
                fp32 bar.  E / E_y reaches 42 (g_bv), which is why fp32's bar is not precision 1's.
  g_bqkv's key third: E / E_y at most 1.75, E / bar at most 0.16.  The packed attention entry points: at most 0.093 of the 1e-5 row bar.
"""
import ctypes as C
import functools

import pytest
import torch

import _train_ref as T

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE = -1, -2
CANARY = 0x5A5A5A5A            # as fp32: 1.5e16
STRIP = 64                     # floats: 256 bytes
GRAD_BUFS = ("dx",) + T.GRADS
FP32_ONLY = ("P", "g_ln2_b")   # precision 1: the tensors whose bf16-operand yardstick has no error at all (this file's docstring)
N_SUMS = 8                     # column sums a backward appends: g_bqkv, g_bo, g_b1, g_b2 and the two LayerNorm pairs


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from hirest_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def side(dev):
    return torch.cuda.Stream(device=dev)


@pytest.fixture(params=[0, 1], ids=["rows", "tiled"])
def attn_impl(request, lib):
    assert lib.hirest_attention_train_select(request.param) == 0
    try:
        yield request.param
    finally:
        assert lib.hirest_attention_train_select(1) == 0


def _s():
    from hirest_amd import ops
    return ops.stream_ptr()


# ---- the problems and their references (computed once, never modified) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(case):
    return T.exact_score_inputs(*T.CASES[case], T.CASE_SEED[case])


def _flat(acts, dx, grads, W):
    out = {n: acts[n] for n in T.ACTS}
    out["dx"] = dx
    out.update(T.sixteen(grads, W))
    return {n: t.double() for n, t in out.items()}


@functools.lru_cache(maxsize=None)
def _refs(case, drop):
    """{'f64', 'f32', 'bf'}: name -> float64 tensor for the 26 compared tensors (bf only where the case runs precision 1), and 'masks'."""
    B, Tn, H, W, mlp = T.CASES[case]
    params, x, dout = _problem(case)
    masks = T.block_masks(B, Tn, H, W, drop, T.SEEDS)
    run = lambda dtype, bf: T.block_ref_grads(params, x, dout, B, Tn, H, drop, T.SEEDS, dtype, bf16_operands=bf, masks=masks)
    a, dx, g = run(torch.float64, False)
    out = {"f64": _flat(a, dx, g, W), "masks": masks}
    out["f32"] = _flat(*run(torch.float32, False), W)
    if 1 in T.PRECISIONS[case]:
        out["bf"] = _flat(*run(torch.float64, True), W)
    return out


# ---- device side ------------------------------------------------------------------------------------------------------------------------
class Arena:
    """One device allocation; every buffer starts on a 256-byte boundary with at least STRIP floats of CANARY between it and its
    neighbours (and the ends of the allocation)."""

    def __init__(self, dev, sizes):
        self.at, off = {}, STRIP
        for name, n in sizes:
            if n > 0:
                self.at[name] = (off, n)
                off = (off + n + STRIP + 63) // 64 * 64
        self.buf = torch.empty((off,), dtype=torch.float32, device=dev)
        self.buf.view(torch.int32).fill_(CANARY)
        self.owned = torch.zeros((off,), dtype=torch.bool)
        for o, n in self.at.values():
            self.owned[o:o + n] = True

    def t(self, name):
        o, n = self.at[name]
        return self.buf[o:o + n]

    def ptr(self, name):
        return self.buf.data_ptr() + 4 * self.at[name][0] if name in self.at else None

    def nbytes(self, name):
        return 4 * self.at[name][1] if name in self.at else 0

    def fill_nan(self):
        for name in self.at:
            self.t(name).fill_(float("nan"))

    def check(self):
        bits = self.buf.view(torch.int32).cpu()
        bad = (bits != CANARY) & ~self.owned
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            near = [n for n, (o, k) in self.at.items() if o - 2 * STRIP <= i < o + k + 2 * STRIP]
            raise AssertionError(f"{int(bad.sum())} floats written outside every buffer, the first at arena offset {i} (next to {near})")


class Block:
    """One block problem on the device: descriptor, arena, and `n_bwd` sets of gradient buffers + backward scratch."""

    def __init__(self, dev, lib, case, precision, drop, n_bwd=1, presplit=False, heads=None):
        from hirest_amd import _lib
        self._lib, self.lib, self.precision = _lib, lib, precision
        B, Tn, H, W, mlp = T.CASES[case]
        H = heads or H
        R = B * Tn
        self.dims = (B, Tn, H, W, mlp, R)
        params, x, dout = _problem(case)
        self.inp = {n: t.to(dev) for n, t in params.items()}
        self.inp["x"], self.inp["dout"] = x.to(dev), dout.to(dev)
        d = _lib.TrainBlock()
        d.struct_size = C.sizeof(_lib.TrainBlock)
        d.B, d.T, d.heads, d.width, d.mlp, d.precision = B, Tn, H, W, mlp, precision
        d.ln_eps, d.drop = 1e-12, float(drop)
        d.seed_attn, d.seed_ao, d.seed_out = T.SEEDS
        for n in T.PARAMS + ("x",):
            setattr(d, n, self.inp[n].data_ptr())
        self.d = d
        self.fwd_need = lib.hirest_train_block_forward_scratch_bytes(C.byref(d))
        self.bwd_need = lib.hirest_train_block_backward_scratch_bytes(C.byref(d))
        assert self.fwd_need % 4 == 0 and self.bwd_need % 4 == 0
        ws_f = max(lib.hirest_gemm_f32_workspace_bytes(R, n, k) for n, k in ((3 * W, W), (W, W), (mlp, W), (W, mlp)))
        ws_b = max(lib.hirest_gemm_f32_layouts_workspace_bytes(R, n, k) for n, k in ((mlp, W), (W, mlp), (W, W), (W, 3 * W)))
        ws_s = max(lib.hirest_gemm_f32_layouts_workspace_bytes(m, n, R) for m, n in ((W, mlp), (mlp, W), (W, W), (3 * W, W)))
        self.act_sizes = dict(qkv=R * 3 * W, P=B * H * Tn * Tn, cx=R * W, a_pre=R * W, aa=R * W, hpre=R * mlp, hh=R * mlp, x_pre=R * W, out=R * W)
        self.grad_sizes = dict(dx=R * W, g_wqkv=3 * W * W, g_bqkv=3 * W, g_wo=W * W, g_bo=W, g_ln1_g=W, g_ln1_b=W, g_w1=mlp * W, g_b1=mlp,
                               g_w2=W * mlp, g_b2=W, g_ln2_g=W, g_ln2_b=W)
        sizes = list(self.act_sizes.items()) + [("out2", R * W if precision == 1 else 0), ("fwd_scratch", self.fwd_need // 4),
                                                ("ws", max(ws_f, ws_b) // 4), ("side_ws", ws_s // 4)]
        for k in range(n_bwd):
            sizes += [(f"{n}.{k}", sz) for n, sz in self.grad_sizes.items()] + [(f"bwd_scratch.{k}", self.bwd_need // 4)]
        self.arena = ar = Arena(dev, sizes)
        for n in T.ACTS:
            setattr(d, n, ar.ptr(n))
        d.out2 = ar.ptr("out2")
        self.split = {}
        if presplit:
            assert precision == 1
            bf = lambda r, c: torch.full((r, c), float("nan"), dtype=torch.bfloat16, device=dev)
            self.split["x2"] = bf(R, 2 * W)
            assert lib.hirest_split2_bf16(self.inp["x"].data_ptr(), W, self.split["x2"].data_ptr(), 2 * W, R, W, 0, _s()) == 0
            for n, (O, I) in dict(wqkv=(3 * W, W), wo=(W, W), w1=(mlp, W), w2=(W, mlp)).items():
                a, b = bf(O, 2 * I), bf(I, 2 * O)
                assert lib.hirest_split2_bf16(self.inp[n].data_ptr(), I, a.data_ptr(), 2 * I, O, I, 0, _s()) == 0
                assert lib.hirest_split2_transposed_bf16(self.inp[n].data_ptr(), I, b.data_ptr(), 2 * O, O, I, _s()) == 0
                self.split[n + "2"], self.split[n + "T2"] = a, b
            for n, t in self.split.items():
                setattr(d, n, t.data_ptr())
        self.tables = [((_lib.ColsumItem * 64)(), C.c_int32(0)) for _ in range(n_bwd)]
        ar.fill_nan()

    def forward(self, use_ws=True, scratch_bytes=None):
        ar, d = self.arena, self.d
        d.ws, d.ws_bytes = (ar.ptr("ws"), ar.nbytes("ws")) if use_ws else (None, 0)
        return self.lib.hirest_train_block_forward(C.byref(d), ar.ptr("fwd_scratch"), self.fwd_need if scratch_bytes is None else scratch_bytes, _s())

    def backward(self, k=0, side=None, use_ws=True, max_items=64, scratch_bytes=None):
        """Enqueues one backward into gradient set k; its column sums wait in self.tables[k] for colsums(k)."""
        ar, d = self.arena, self.d
        d.ws, d.ws_bytes = (ar.ptr("ws"), ar.nbytes("ws")) if use_ws else (None, 0)
        g = self._lib.TrainBlockGrads()
        g.struct_size = C.sizeof(self._lib.TrainBlockGrads)
        g.dout = self.inp["dout"].data_ptr()
        for n in GRAD_BUFS:
            setattr(g, n, ar.ptr(f"{n}.{k}"))
        items, count = self.tables[k]
        g.items, g.n_items, g.max_items = items, C.pointer(count), max_items
        if side is not None:
            g.side_stream = side.cuda_stream
            g.side_ws, g.side_ws_bytes = (ar.ptr("side_ws"), ar.nbytes("side_ws")) if use_ws else (None, 0)
        g.scratch, g.scratch_bytes = ar.ptr(f"bwd_scratch.{k}"), self.bwd_need if scratch_bytes is None else scratch_bytes
        return self.lib.hirest_train_block_backward(C.byref(d), C.byref(g), _s())

    def colsums(self, k=0):
        items, count = self.tables[k]
        assert count.value == N_SUMS, count.value
        assert self.lib.hirest_weighted_colsum_grouped_f32(items, count.value, _s()) == 0
        count.value = 0

    def join(self, side=None):
        if side is not None:
            side.synchronize()
        torch.cuda.synchronize()

    def results(self, k=0, acts=True):
        """CPU copies (every one free of NaN) of the kept activations (+ out2's bits in precision 1) and of gradient set k."""
        ar = self.arena
        B, Tn, H, W, mlp, R = self.dims
        shapes = dict(qkv=(R, 3 * W), P=(B, H, Tn, Tn), hpre=(R, mlp), hh=(R, mlp), g_wqkv=(3 * W, W), g_wo=(W, W), g_w1=(mlp, W), g_w2=(W, mlp))
        out = {}
        for n in (T.ACTS if acts else ()) + GRAD_BUFS:
            t = ar.t(n if n in T.ACTS else f"{n}.{k}").cpu()
            assert not bool(torch.isnan(t).any()), f"{n}: {int(torch.isnan(t).sum())} of {t.numel()} elements were never written"
            out[n] = t.view(shapes.get(n, (R, W) if t.numel() == R * W and n not in T.GRADS else (-1,)))
        if acts and self.precision == 1:
            o2 = ar.t("out2").cpu().view(torch.bfloat16)
            assert not bool(torch.isnan(o2.float()).any()), "out2"
            out["out2"] = o2.view(torch.int16)
        return out


def _run(dev, lib, case, precision, drop, side=None, use_ws=True, presplit=False):
    """Forward + backward + column sums of one block; checks the arena's pattern; returns (results, the Block)."""
    blk = Block(dev, lib, case, precision, drop, presplit=presplit)
    assert blk.fwd_need > 0 and blk.bwd_need > 0, "the scratch size functions refuse a case that block_ok() admits"
    assert blk.forward(use_ws) == 0, "train_block_forward"
    assert blk.backward(0, side, use_ws) == 0, "train_block_backward"
    blk.colsums(0)
    blk.join(side)
    blk.arena.check()
    return blk.results(0), blk


def _same(a, b, what):
    assert set(a) == set(b)
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs in {int((a[n] != b[n]).sum())} of {a[n].numel()} elements"


# ---- against fp64 ---------------------------------------------------------------------------------------------------------------------
def _compare(case, precision, drop, got, what):
    B, Tn, H, W, mlp = T.CASES[case]
    ref = _refs(case, drop)
    r64, r32, rbf = ref["f64"], ref["f32"], ref.get("bf")
    g = _flat(got, got["dx"], got, W)
    fails, worst = [], (0.0, None)
    for n in r64:
        err = (g[n] - r64[n]).abs()
        E, E_y, top = err.max().item(), (r32[n] - r64[n]).abs().max().item(), r64[n].abs().max().item()
        bar = 4 * E_y + 2.0 ** -23 * top
        E_bf = (rbf[n] - r64[n]).abs().max().item() if precision == 1 else None
        if n == "g_bk":                  # zero in exact arithmetic: the yardstick's own floor, on the scale of the tensor it is a third of
            bar = 4 * E_y + 2.0 ** -23 * max(r64[m].abs().max().item() for m in ("g_bq", "g_bk", "g_bv"))
        elif precision == 1:
            assert (E_bf == 0) == (n in FP32_ONLY), f"{what}: E_bf of {n} is {E_bf:.3g}"
            if E_bf > 0:
                bar = E_bf / 50
        ratio = E / bar if bar > 0 else (0.0 if E == 0 else float("inf"))
        print(f"{what} {n}: E {E:.3g}  E/E_y {E / E_y if E_y else float('nan'):.3g}" +
              (f"  E/E_bf {E / E_bf if E_bf else float('nan'):.3g}" if precision == 1 else "") + f"  E/bar {ratio:.3g}")
        if ratio > worst[0]:
            worst = (ratio, n)
        if not ratio <= 1.0:
            fails.append((n, E, bar))
    print(f"{what}: worst E/bar {worst[0]:.3g} ({worst[1]})")
    # P: zero nowhere the reference is not
    lost = (got["P"] == 0) & (r64["P"] != 0)
    assert not bool(lost.any()), f"{what}: P is exactly zero at {int(lost.sum())} positions where the reference is not"
    # the two residual dropouts: exactly the restated masks
    x = _problem(case)[1]
    _, keep_ao, keep_out = ref["masks"]
    for name, diff, keep, base, upd in (("a_pre - x", got["a_pre"] - x, keep_ao, x.double(), r64["a_pre"] - x.double()),
                                        ("x_pre - aa", got["x_pre"] - got["aa"], keep_out, r64["aa"], r64["x_pre"] - r64["aa"])):
        dropped = keep == 0
        assert bool((diff[dropped] == 0).all()), f"{what}: {name} is non-zero at {int((diff[dropped] != 0).sum())} dropped positions"
        visible = ~dropped & (upd.abs() > 2.0 ** -20 * base.abs())
        assert bool((diff[visible] != 0).all()), f"{what}: {name} is zero at {int((diff[visible] == 0).sum())} kept positions"
        assert drop > 0 or not bool(dropped.any())
    assert not fails, f"{what}: " + "; ".join(f"{n}: E {E:.3g} > bar {bar:.3g}" for n, E, bar in fails)


CASE_PRECISION = [(c, p) for c in T.CASES for p in T.PRECISIONS[c]]


@pytest.mark.parametrize("drop", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("case,precision", CASE_PRECISION)
def test_block_against_fp64(dev, lib, side, attn_impl, case, precision, drop):
    """Every kept activation, dx and the sixteen gradients against block_ref / block_ref_grads in fp64 at the bars of this file's
    docstring, with the weight-gradient products on the side stream and the fp32 GEMMs' workspace given."""
    got, _ = _run(dev, lib, case, precision, drop, side=side)
    _compare(case, precision, drop, got, f"{case} p{precision} drop {drop} impl {attn_impl}")


@pytest.mark.parametrize("precision", [0, 1])
def test_block_is_bit_identical_across_its_options(dev, lib, side, precision):
    """Case x3, drop 0.1: side stream or not, pre-split operands or not (precision 1), a second run into fresh buffers; case split:
    with the fp32 GEMMs' workspace (the split form of the 1024-deep product) and without."""
    base, _ = _run(dev, lib, "x3", precision, 0.1, side=side)
    _same(base, _run(dev, lib, "x3", precision, 0.1, side=None)[0], "single stream")
    _same(base, _run(dev, lib, "x3", precision, 0.1, side=side)[0], "second run")
    if precision == 1:
        _same(base, _run(dev, lib, "x3", 1, 0.1, side=side, presplit=True)[0], "pre-split x2 and weights")
    B, Tn, H, W, mlp = T.CASES["split"]
    if precision == 0:
        assert lib.hirest_gemm_f32_workspace_bytes(B * Tn, W, mlp) > 0, "case split does not reach the split form"
    with_ws, blk = _run(dev, lib, "split", precision, 0.1, side=side)
    assert precision == 1 or blk.arena.nbytes("ws") > 0
    _same(with_ws, _run(dev, lib, "split", precision, 0.1, side=side, use_ws=False)[0], "ws = NULL")


@pytest.mark.parametrize("case,precision", [("odd", 0), ("x3", 0), ("x3", 1)])
def test_block_writes_only_its_buffers(dev, lib, side, case, precision):
    """Scratch of exactly *_scratch_bytes(), every buffer between 256-byte strips of a bit pattern inside one arena: after forward and
    backward (drop 0.5, side stream) every strip is intact and no output element is still NaN.  (A scratch plan that under-counts a
    slice at a width or mlp other than 768 / 3072 writes into a strip.)"""
    blk = Block(dev, lib, case, precision, 0.5)
    assert blk.arena.at["fwd_scratch"][1] * 4 == blk.fwd_need and blk.arena.at["bwd_scratch.0"][1] * 4 == blk.bwd_need
    assert blk.forward() == 0
    blk.join()
    blk.arena.check()
    assert blk.backward(0, side) == 0
    blk.colsums(0)
    blk.join(side)
    blk.arena.check()
    blk.results(0)


@pytest.mark.parametrize("precision", [0, 1])
def test_side_stream_event_ring_reuse(dev, lib, side, precision):
    """20 backwards enqueued back to back without synchronisation: 80 weight-gradient products on the side stream behind 80 event
    records, more than the 64 events of train_block.hip's ring, so events are re-recorded while earlier waits on them may still be
    pending.  Every one of the 20 result sets equals the single-stream result bit for bit."""
    n = 20
    want, _ = _run(dev, lib, "x3", precision, 0.1, side=None)
    blk = Block(dev, lib, "x3", precision, 0.1, n_bwd=n)
    assert blk.forward() == 0
    for k in range(n):
        assert blk.backward(k, side) == 0
    for k in range(n):
        blk.colsums(k)
    blk.join(side)
    blk.arena.check()
    for k in range(n):
        got = blk.results(k, acts=False)
        _same(got, {m: want[m] for m in got}, f"backward {k} of {n}")


# ---- the packed-qkv attention entry points the block calls -------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", ["one", "odd", "x3"])
def test_packed_attention_entry_points_against_fp64(dev, lib, attn_impl, case, p):
    """hirest_attention_train_fwd_f32 / _bwd_f32 with add_const = -10000 on the qkv of the builder's cases: P, ctx, dS and dqkv against
    fp64 autograd within 1e-5 of the row's scale, the bar test_attention_train_vs_fp64 holds the general forms to at add_const = 0
    (row: a score row of P / dS, the 64 dimensions of one head of ctx / dq / dk / dv).  It holds with the constant present because
    the scores are exact: fl32(s - 10000) is the same number in the kernel and in the reference."""
    B, Tn, H, W, mlp = T.CASES[case]
    R = B * Tn
    params, x, dout = _problem(case)
    qkv = x @ params["wqkv"].t() + params["bqkv"]
    seed = T.SEEDS[0]
    keep = T.block_masks(B, Tn, H, W, p, (seed, 0, 0))[0]
    q64 = qkv.double().requires_grad_(True)
    S, P64, cx64 = T.attention(q64, B, Tn, H, keep.double())
    S.retain_grad()
    cx64.backward(dout.double())
    qd, dd = qkv.to(dev), dout.to(dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    P, ctx, dS, dqkv = nan(B, H, Tn, Tn), nan(R, W), nan(B, H, Tn, Tn), nan(R, 3 * W)
    assert lib.hirest_attention_train_fwd_f32(qd.data_ptr(), P.data_ptr(), ctx.data_ptr(), B, Tn, H, 64, 0.125, T.ADD_CONST, p, seed, _s()) == 0
    assert lib.hirest_attention_train_bwd_f32(qd.data_ptr(), P.data_ptr(), dd.data_ptr(), dS.data_ptr(), dqkv.data_ptr(), B, Tn, H, 64, 0.125,
                                              p, seed, _s()) == 0
    what = f"packed attention {case} p={p} impl={attn_impl}"
    for name, got, ref in (("P", P, P64.detach()), ("dS", dS, S.grad), ("ctx", ctx.view(-1, 64), cx64.detach().reshape(-1, 64)),
                           ("dqkv", dqkv.view(-1, 64), q64.grad.reshape(-1, 64))):
        got = got.cpu()
        assert not bool(torch.isnan(got).any()), f"{what}: {name} has elements that were never written"
        T._rows_close(got, ref, 1e-5, f"{what} {name}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_block_refusals(dev, lib, side):
    """Host-side returns, nothing faults: a column-sum table one item short (a backward appends eight sums — g_bqkv is one of them, not
    three — so max_items = 7 is HIREST_E_BADARG once the eighth is appended: the launches before it are enqueued, so synchronise;
    max_items = 8 is enough), precision 1 at a width / mlp that is no multiple of 32 (HIREST_E_SHAPE from both
    directions), a scratch one byte short, and a width that the heads do not divide."""
    blk = Block(dev, lib, "x3", 0, 0.1)
    assert blk.forward(scratch_bytes=blk.fwd_need - 1) == E_BADARG
    assert blk.forward() == 0
    assert blk.backward(0, side, scratch_bytes=blk.bwd_need - 1) == E_BADARG
    assert blk.tables[0][1].value == 0
    assert blk.backward(0, side, max_items=N_SUMS - 1) == E_BADARG
    blk.join(side)
    assert blk.tables[0][1].value == N_SUMS - 1
    blk.tables[0][1].value = 0
    assert blk.backward(0, side, max_items=N_SUMS) == 0
    blk.colsums(0)
    blk.join(side)
    blk.results(0)
    blk.arena.check()
    odd = Block(dev, lib, "odd", 1, 0.1)
    assert odd.fwd_need > 0 and odd.bwd_need > 0
    assert odd.forward() == E_SHAPE
    assert odd.backward(0, side) == E_SHAPE
    odd.join(side)
    assert odd.tables[0][1].value == 0
    assert bool(torch.isnan(odd.arena.t("qkv")).all()) and bool(torch.isnan(odd.arena.t("dx.0")).all())
    bad = Block(dev, lib, "x3", 0, 0.1, heads=5)                       # 128 % 5 != 0
    assert bad.fwd_need == 0 and bad.bwd_need == 0
    assert bad.forward() == E_BADARG and bad.backward(0, side) == E_BADARG
    bad.join(side)
