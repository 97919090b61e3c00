"""The exact-fp32 GEMM family (csrc/joint.hip) held to the bit, with padded strides, NaN padding and guarded outputs.

Operands are integers (tests/_exact_inputs.py gemm_f32_exact; preconditions in tests/test_exact_inputs_host.py) bounded so that
sum_k |a| |w| + 24 < 2^24: fp32 accumulation is exact in any order, so every kernel, K-quarter order and split has one right bit
pattern — the fp64 product cast to fp32, compared with torch.equal.  A dropped k, a slab read twice or a wrong m % period row is a
hard failure.

Every call
  * pads every stride (lda = K + 12, ldw = K + 8, ldr = N + 4, ldo = N + 12) and fills the input padding with NaN,
  * writes into a sentinel-filled buffer with one guard row before and after the output, and asserts that every sentinel (pad columns
    and guard rows) is unchanged bit for bit,
  * asks hirest_gemm_f32_dispatch_name first (current switches, the device's CU count) and asserts the kernel it means to test; the
    same names at 256 CUs are checked without a GPU in test_exact_inputs_host.py, together with the fact that the lists reach every
    instantiation.

Activations 1 - 3 are not exact.  max |got - fp64 act(x)| over exact pre-activations x (gemm_f32_act) is held to 4 times the error
of the same formula evaluated in fp32 by torch on the CPU (the resid and periodic addends are integers added after the activation:
a wrong order fails by whole units).  Next to addends of up to 16 the rounding of the two additions is most of both errors (1.0e-6 ..
1.4e-6), so every case also runs without them, where the activation's own error is what is measured.  Measured ratio got / CPU on the
MI355X, the same on all four kernels (tile64, tile64.split, m16<2,1,6>, skinny):
  with addends   gelu (erf) 1.00   tanh 1.00   quick-gelu 1.00
  bare           gelu (erf) 1.00   tanh 1.68 (5.0e-8 against 3.0e-8)   quick-gelu 1.00

The LayerNorm forms cannot take integers; they are held to the bits of hirest_layernorm + hirest_gemm_f32 on the same padded
operands, the second half of which the exact tests verify.

Overlapping A (lda < K, the Whisper stem's convolutions as GEMMs): the view sits in a NaN-filled buffer, so a NaN anywhere in `out`
means a value outside the view reached a product.  This cannot show that no ADDRESS outside the view is touched (a load whose value
is discarded leaves no trace); that rests on the clamps below, which keep every load of row m inside [A + m lda, A + m lda + K):
  tile64        rows: gm = min(M0 + srow, M - 1); k: 4-vectors at k0 + sk + 4 h < K, else re-read at K - 4 (gemm_f32_kernel fetch)
  tile64.split  the same kernel; a block fetches the slabs of its own K quarter only (s_first .. s_last)
  ring<4>       rows: gm = min(M0 + r, M - 1); K % 32 == 0 and slabs s < nslab = K / 32 only, 128 B each
  skinny        rows: gm = min(M0 + row, M - 1); a 4-vector is loaded only under `s < cnt && k0 + 16 khalf + 4 h < K`
  m16<..>       rows: gm = min(.., M - 1); K % 32 == 0; slab index first + min(s, cnt - 1) < nslab, issued only when cnt > 0
  rows, m16ln*  read X / A rows at a clamped row index and exactly K = 768 (256 NV) floats of it"""
import ctypes as C
from contextlib import contextmanager

import pytest
import torch

import _exact_inputs as X

pytestmark = pytest.mark.gpu

SENT = 0x4B1DE5A5            # fp32 sentinel bits: a finite value (10 347 941) no result here equals
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib
    return _lib.load()


@contextmanager
def switches(lib, select_kernel=0, ring_mode=0, rows_ln_mode=2):
    from hirest_amd import _lib
    try:
        _lib.check(lib.hirest_gemm_f32_select_kernel(select_kernel), "select_kernel")
        _lib.check(lib.hirest_gemm_f32_ring_mode(ring_mode), "ring_mode")
        _lib.check(lib.hirest_gemm_f32_rows_ln_mode(rows_ln_mode), "rows_ln_mode")
        yield
    finally:
        lib.hirest_gemm_f32_select_kernel(0)
        lib.hirest_gemm_f32_ring_mode(0)
        lib.hirest_gemm_f32_rows_ln_mode(2)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _expect(lib, name, entry, M, N, K, **fields):
    """The dispatch decision of this process (current switches) on this device must be `name`."""
    from hirest_amd import _lib
    buf = C.create_string_buffer(64)
    q = _lib.GemmF32Query.make(entry, M, N, K, **fields)
    _lib.check(lib.hirest_gemm_f32_dispatch_name(C.byref(q), buf, 64), "hirest_gemm_f32_dispatch_name")
    assert buf.value.decode() == name, (entry, M, N, K, fields)


def _padded(t, ld, dev):
    """[rows, ld] on the device: t in the first columns, NaN in the rest."""
    buf = torch.full((t.shape[0], ld), NAN, dtype=torch.float32, device=dev)
    buf[:, :t.shape[1]] = t
    return buf


def _sentinel(shape, dev):
    return torch.full(shape, SENT, dtype=torch.int32, device=dev).view(torch.float32)


class Guarded:
    """[rows, cols] inside a sentinel-filled [rows + 2, ld] buffer: one guard row before and after, ld - cols pad columns."""

    def __init__(self, rows, cols, ld, dev):
        self.rows, self.cols = rows, cols
        self.buf = _sentinel((rows + 2, ld), dev)
        self.view = self.buf[1:rows + 1]

    def result(self):
        """The [rows, cols] result, after asserting that every sentinel around it has kept its bits."""
        bits = self.buf.view(torch.int32)
        assert bool((bits[0] == SENT).all()), "guard row before the output was written"
        assert bool((bits[self.rows + 1] == SENT).all()), "guard row after the output was written"
        assert bool((bits[1:self.rows + 1, self.cols:] == SENT).all()), "pad columns of the output were written"
        return self.view[:, :self.cols]


_DEV = {}


def _operands(kind, M, N, K, dev):
    """Generator output of a shape on the device with padded strides; the last shape is kept."""
    key = (kind, M, N, K)
    if key not in _DEV:
        _DEV.clear()
        d = dict(X.gemm_f32_exact(M, N, K) if kind == "exact" else X.gemm_f32_act(M, N, K))
        d["A"], d["W"] = _padded(d["a"], K + 12, dev), _padded(d["w"], K + 8, dev)
        d["R"] = _padded(d["resid"], N + 4, dev)
        d["bias_d"], d["periodic_d"] = d["bias"].to(dev), d["periodic"].to(dev)
        _DEV[key] = d
    return _DEV[key]


def _call(lib, dev, name, entry, A, lda, W, ldw, M, N, K, bias=None, resid=None, ldr=0, periodic=None, period=0, act=0, colmax=False):
    """One call of a plain entry point ("gemm", "ws", "rows_colmax") into a guarded output; returns (out [M, N], colmax or None)."""
    from hirest_amd import _lib, ops
    ldo = N + 12
    out = Guarded(M, N, ldo, dev)
    s = ops.stream_ptr()
    fields = dict(has_resid=resid is not None, has_periodic=periodic is not None, has_workspace=entry == "ws")
    _expect(lib, name, entry, M, N, K, **fields)
    cm = None
    if entry == "gemm":
        _lib.check(lib.hirest_gemm_f32(_ptr(A), lda, _ptr(W), ldw, _ptr(bias), _ptr(resid), ldr, _ptr(periodic), period, _ptr(out.view), ldo,
                                       M, N, K, act, s), "hirest_gemm_f32")
    elif entry == "ws":
        need = lib.hirest_gemm_f32_workspace_bytes(M, N, K)
        assert need == 16 * M * N
        ws = _sentinel((need // 4 + 64,), dev)                         # 64 canary floats past workspace_bytes
        _lib.check(lib.hirest_gemm_f32_ws(_ptr(A), lda, _ptr(W), ldw, _ptr(bias), _ptr(resid), ldr, _ptr(periodic), period, _ptr(out.view), ldo,
                                          M, N, K, act, _ptr(ws), need, s), "hirest_gemm_f32_ws")
        assert bool((ws[need // 4:].view(torch.int32) == SENT).all()), "the split form wrote past workspace_bytes"
    else:
        ntile = (N + 15) // 16
        cmg = Guarded(M, ntile, ntile, dev) if colmax else None
        _lib.check(lib.hirest_gemm_f32_rows_colmax(_ptr(A), lda, _ptr(W), ldw, _ptr(bias), _ptr(out.view), ldo,
                                                   _ptr(cmg.view) if colmax else None, M, N, K, s), "hirest_gemm_f32_rows_colmax")
        cm = cmg.result() if colmax else None
    return out.result(), cm


def _exact_ref(d, M, bias, resid, period):
    ref = d["ref"].clone()
    if bias:
        ref += d["bias"].double()
    if resid:
        ref += d["resid"].double()
    if period:
        ref += d["periodic"][torch.arange(M) % period].double()
    return ref.float()                                                 # exact: an integer below 2^24


def _tile_max(ref):
    """Per row, the maximum of each 16-column tile of ref, the ragged last tile padded with -inf."""
    M, N = ref.shape
    ntile = (N + 15) // 16
    pad = torch.full((M, ntile * 16), float("-inf"), dtype=ref.dtype)
    pad[:, :N] = ref
    return pad.reshape(M, ntile, 16).amax(-1)


def _run_exact(lib, dev, name, entry, M, N, K, combos):
    d = _operands("exact", M, N, K, dev)
    for bias, resid, period in combos:
        got, _ = _call(lib, dev, name, entry, d["A"], K + 12, d["W"], K + 8, M, N, K, bias=d["bias_d"] if bias else None,
                       resid=d["R"] if resid else None, ldr=N + 4 if resid else 0, periodic=d["periodic_d"] if period else None, period=period)
        assert torch.equal(got.cpu(), _exact_ref(d, M, bias, resid, period)), (name, M, N, K, bias, resid, period)


PLAIN_CASES = [(name, entry, sel, ring, s) for name, entry, sel, ring, shapes in X.F32_PLAIN for s in shapes]


@pytest.mark.parametrize("name,entry,sel,ring,shape", PLAIN_CASES, ids=[f"{c[0]}-{c[2]}{c[3]}-{'x'.join(map(str, c[4]))}" for c in PLAIN_CASES])
def test_exact_at_kernel_edges(lib, dev, name, entry, sel, ring, shape):
    """a w^T + bias + resid + periodic[m % 7], and the bare product, bit for bit.  On one shape per kernel family every operand alone and
    the periods 1, M and M + 3 as well (period 7 on rows past a tile boundary shows a wrong m % period)."""
    M, N, K = shape
    combos = [(True, True, 7), (False, False, 0)]
    if X.F32_EPILOGUE.get(name) == shape:
        combos += [(True, False, 0), (False, True, 0), (False, False, 7), (False, False, 1), (False, False, M), (True, True, M + 3)]
    with switches(lib, select_kernel=sel, ring_mode=ring):
        _run_exact(lib, dev, name, entry, M, N, K, combos)


def test_every_family_has_its_epilogue_shape():
    for name, shape in X.F32_EPILOGUE.items():
        assert any(n == name and shape in shapes for n, _, _, _, shapes in X.F32_PLAIN), name


@pytest.mark.parametrize("name,entry,shape", X.F32_ROWS, ids=[f"{n}-{e}-{'x'.join(map(str, s))}" for n, e, s in X.F32_ROWS])
def test_exact_rows_stream(lib, dev, name, entry, shape):
    """The row-group streaming kernel: with and without bias, and the per-tile row maxima next to a sentinel row."""
    M, N, K = shape
    d = _operands("exact", M, N, K, dev)
    with switches(lib):
        for bias in (True, False):
            got, cm = _call(lib, dev, name, entry, d["A"], K + 12, d["W"], K + 8, M, N, K, bias=d["bias_d"] if bias else None, colmax=True)
            ref = _exact_ref(d, M, bias, False, 0)
            assert torch.equal(got.cpu(), ref), (shape, bias)
            if cm is not None:
                assert torch.equal(cm.cpu(), _tile_max(ref)), (shape, bias)


@pytest.mark.parametrize("name,ak,wk", X.F32_LAYOUTS, ids=[n for n, _, _ in X.F32_LAYOUTS])
def test_exact_layouts(lib, dev, name, ak, wk):
    """hirest_gemm_f32_layouts with either operand k-major: the k-major operand is [K, rows + pad] with NaN in the pad columns."""
    from hirest_amd import _lib, ops
    M, N, K = X.F32_LAYOUT_SHAPE
    d = _operands("exact", M, N, K, dev)
    A, lda = (_padded(d["a"].t().contiguous(), M + 12, dev), M + 12) if ak else (d["A"], K + 12)
    W, ldw = (_padded(d["w"].t().contiguous(), N + 8, dev), N + 8) if wk else (d["W"], K + 8)
    ldo, ldr = N + 12, N + 4
    for bias, resid in ((True, True), (False, False)):
        out = Guarded(M, N, ldo, dev)
        _expect(lib, name, "layouts", M, N, K, a_kmajor=ak, w_kmajor=wk, has_resid=resid)
        _lib.check(lib.hirest_gemm_f32_layouts(_ptr(A), lda, ak, _ptr(W), ldw, wk, _ptr(d["bias_d"]) if bias else None, _ptr(d["R"]) if resid else None,
                                               ldr if resid else 0, _ptr(out.view), ldo, M, N, K, 0, None, 0, ops.stream_ptr()), "hirest_gemm_f32_layouts")
        assert torch.equal(out.result().cpu(), _exact_ref(d, M, bias, resid, 0)), (name, bias, resid)


ACT_CASES = [(name, entry, sel, shape, act) for name, entry, sel, shape in X.F32_ACT for act in (1, 2, 3)]


@pytest.mark.parametrize("name,entry,sel,shape,act", ACT_CASES, ids=[f"{c[0]}-act{c[4]}" for c in ACT_CASES])
def test_activations_against_fp64(lib, dev, name, entry, sel, shape, act):
    """act(a w^T + bias) + resid + periodic[m % 7], and act(a w^T + bias) alone: next to integer addends of up to 16 the rounding of the two
    additions (half an ulp of 16 each) is most of both errors, so the second call holds the activation's own error to the same bar."""
    M, N, K = shape
    d = _operands("act", M, N, K, dev)
    rows = torch.arange(M) % 7
    for addends in (True, False):
        ref, cpu = X.f32_act(d["x"], act), X.f32_act(d["x"].float(), act)
        if addends:
            ref = ref + d["resid"].double() + d["periodic"][rows].double()
            cpu = (cpu + d["resid"]) + d["periodic"][rows]                                     # the epilogue's order, in fp32
        with switches(lib, select_kernel=sel):
            got, _ = _call(lib, dev, name, entry, d["A"], K + 12, d["W"], K + 8, M, N, K, bias=d["bias_d"], resid=d["R"] if addends else None,
                           ldr=N + 4 if addends else 0, periodic=d["periodic_d"] if addends else None, period=7 if addends else 0, act=act)
        err_got, err_cpu = (got.cpu().double() - ref).abs().max().item(), (cpu.double() - ref).abs().max().item()
        print(f"act {act} {name} {'with addends' if addends else 'bare'}: max |got - fp64| {err_got:.3e}, torch fp32 on the CPU {err_cpu:.3e}, "
              f"ratio {err_got / err_cpu:.2f}")
        assert err_cpu > 0 and err_got <= 4 * err_cpu, (addends, err_got, err_cpu)


@pytest.mark.parametrize("lda,K,M,entry,sel,ring,name", X.F32_OVERLAP, ids=[f"{c[6]}-lda{c[0]}-K{c[1]}-M{c[2]}-{c[4]}{c[5]}" for c in X.F32_OVERLAP])
def test_exact_with_overlapping_rows_of_a(lib, dev, lda, K, M, entry, sel, ring, name):
    """A[m, k] = buf[offset + m lda + k] with lda < K, NaN all around the view: the gathered product, bit for bit, and no NaN."""
    N = X.F32_OVERLAP_N
    buf, off, gathered = X.overlap_view(M, lda, K)
    w = X.gemm_f32_exact(N, N, K)["w"]                                 # [N, K] integers in [-15, 15]
    bias = X.gemm_f32_exact(N, N, K)["bias"]
    ref = (gathered.double() @ w.double().t() + bias.double()).float()
    buf_d, W = buf.to(dev), _padded(w, K + 8, dev)
    with switches(lib, select_kernel=sel, ring_mode=ring):
        got, _ = _call(lib, dev, name, entry, buf_d[off:], lda, W, K + 8, M, N, K, bias=bias.to(dev))
    got = got.cpu()
    assert not bool(torch.isnan(got).any()), "a value outside the view reached a product"
    assert torch.equal(got, ref)


# ---- the LayerNorm forms: same bits as hirest_layernorm + hirest_gemm_f32 on the same padded operands


def _ln_inputs(M, N, K, dev, ids):
    from hirest_amd import synth
    x = synth.tensor(f"f32ln.x.{M}.{K}", (M, K), 1.0, 3)
    x[:, 1::7] *= 8.0
    d = {"w": synth.tensor(f"f32ln.w.{N}.{K}", (N, K), 0.05, 4), "bias": synth.tensor(f"f32ln.b.{N}", (N,), 0.5, 5),
         "gamma": 1.0 + synth.tensor(f"f32ln.g.{K}", (K,), 0.2, 6), "beta": synth.tensor(f"f32ln.be.{K}", (K,), 0.2, 7),
         "resid": synth.tensor(f"f32ln.r.{M}.{N}", (M, N), 1.0, 8)}
    d = {k: v.to(dev) for k, v in d.items()}
    if ids:
        vocab = 53
        d["table"] = synth.tensor(f"f32ln.t.{K}", (vocab, K), 1.0, 9).to(dev)
        d["pos_row"] = synth.tensor(f"f32ln.p.{K}", (K,), 0.5, 10).to(dev)
        d["ids"] = ((torch.arange(M) * 7 + 3) % vocab).to(torch.int32).to(dev)
        x = d["table"][d["ids"].long()] + d["pos_row"]                # one fp32 addition per element, as the prologue does it
    d["X"] = _padded(x.to(dev), K + 12, dev)
    d["W"] = _padded(d["w"], K + 8, dev)
    d["R"] = _padded(d["resid"], N + 4, dev)
    return d


def _ln_chain(lib, dev, d, M, N, K, resid):
    """hirest_layernorm, then hirest_gemm_f32 on its output: (ln [M, K], out [M, N])."""
    from hirest_amd import _lib, ops
    s = ops.stream_ptr()
    ldl, ldo = K + 4, N + 12
    ln, out = Guarded(M, K, ldl, dev), Guarded(M, N, ldo, dev)
    _lib.check(lib.hirest_layernorm(_ptr(d["X"]), K + 12, None, _ptr(d["gamma"]), _ptr(d["beta"]), 1e-5, _ptr(ln.view), ldl, 1, M, K, s), "hirest_layernorm")
    _lib.check(lib.hirest_gemm_f32(_ptr(ln.view), ldl, _ptr(d["W"]), K + 8, _ptr(d["bias"]), _ptr(d["R"]) if resid else None, N + 4 if resid else 0,
                                   None, 0, _ptr(out.view), ldo, M, N, K, 0, s), "hirest_gemm_f32")
    return ln.result().clone(), out.result().clone()


def _ln_call(lib, dev, name, d, M, N, K, resid=False, ids=False, ln_out=True, colmax=False):
    """hirest_gemm_f32_ln (or _ln_colmax) into guarded buffers: (ln_out or None, out, colmax or None)."""
    from hirest_amd import _lib, ops
    s = ops.stream_ptr()
    ldl, ldo, ntile = K + 4, N + 12, (N + 15) // 16
    ln, out = Guarded(M, K, ldl, dev), Guarded(M, N, ldo, dev)
    if colmax:
        cm = Guarded(M, ntile, ntile, dev)
        _expect(lib, name, "ln_colmax", M, N, K)
        _lib.check(lib.hirest_gemm_f32_ln_colmax(_ptr(d["X"]), K + 12, _ptr(d["gamma"]), _ptr(d["beta"]), 1e-5, _ptr(d["W"]), K + 8, _ptr(d["bias"]),
                                                 _ptr(out.view), ldo, _ptr(cm.view), M, N, K, s), "hirest_gemm_f32_ln_colmax")
        return None, out.result(), cm.result()
    _expect(lib, name, "ln", M, N, K, has_resid=resid, has_ids=ids, has_ln_out=ln_out)
    _lib.check(lib.hirest_gemm_f32_ln(None if ids else _ptr(d["X"]), K + 12, _ptr(d["ids"]) if ids else None, _ptr(d["table"]) if ids else None,
                                      _ptr(d["pos_row"]) if ids else None, _ptr(d["gamma"]), _ptr(d["beta"]), 1e-5, _ptr(ln.view) if ln_out else None,
                                      ldl if ln_out else 0, _ptr(d["W"]), K + 8, _ptr(d["bias"]), _ptr(d["R"]) if resid else None, N + 4 if resid else 0,
                                      _ptr(out.view), ldo, M, N, K, 0, s), "hirest_gemm_f32_ln")
    ln_res = ln.result()                                               # (without ln_out: every sentinel of the buffer is still checked)
    return (ln_res if ln_out else None), out.result(), None


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name,shape,resid,ids", X.F32_M16LN, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in X.F32_M16LN])
def test_ln_m16_same_bits_as_the_two_calls(lib, dev, name, shape, resid, ids):
    M, N, K = shape
    d = _ln_inputs(M, N, K, dev, ids)
    with switches(lib):
        ln_ref, out_ref = _ln_chain(lib, dev, d, M, N, K, resid)
        ln, out, _ = _ln_call(lib, dev, name, d, M, N, K, resid=resid, ids=ids)
    assert _same_bits(ln, ln_ref) and _same_bits(out, out_ref)


_STREAM = {}


def _stream_ref(lib, dev):
    """Inputs of the largest stream case and the two-call reference on all 32 rows, once: a row's result does not depend on the row count."""
    if not _STREAM:
        N, K = X.F32_STREAM_NK
        d = _ln_inputs(32, N, K, dev, False)
        with switches(lib):
            _, out_ref = _ln_chain(lib, dev, d, 32, N, K, False)
        _STREAM.update(d=d, out=out_ref)
    return _STREAM["d"], _STREAM["out"]


@pytest.mark.parametrize("M,name", X.F32_STREAM, ids=[f"M{m}" for m, _ in X.F32_STREAM])
def test_ln_stream_same_bits_as_the_two_calls(lib, dev, M, name):
    N, K = X.F32_STREAM_NK
    d, out_ref = _stream_ref(lib, dev)
    with switches(lib):
        _, out, _ = _ln_call(lib, dev, name, d, M, N, K, ln_out=False)
        _, out_c, cm = _ln_call(lib, dev, name, d, M, N, K, colmax=True)
    assert _same_bits(out, out_ref[:M]) and _same_bits(out_c, out_ref[:M])
    assert torch.equal(cm.cpu(), _tile_max(out_ref[:M].cpu()))


@pytest.mark.parametrize("mode,shape,name", X.F32_ROWS_LN, ids=[f"{c[2]}-{'x'.join(map(str, c[1]))}" for c in X.F32_ROWS_LN])
def test_ln_rows_same_bits_as_the_two_calls(lib, dev, mode, shape, name):
    M, N, K = shape
    d = _ln_inputs(M, N, K, dev, False)
    with switches(lib, rows_ln_mode=mode):
        ln_ref, out_ref = _ln_chain(lib, dev, d, M, N, K, False)
        ln, out, _ = _ln_call(lib, dev, name, d, M, N, K)
    assert _same_bits(ln, ln_ref) and _same_bits(out, out_ref)
