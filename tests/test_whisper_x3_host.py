"""The bf16x3 precision of the Whisper audio encoder, everything that needs no GPU: the fp64 restatement that is the
yardstick of tests/test_gpu_whisper_x3.py against the committed goldens, set_precision / load_encoder / load_model / the environment
variable, the ABI of csrc/whisper_enc_x3.hip, and the kernel family each of a block's four products takes.

Printed by test_restatement_reproduces_the_goldens (max |ref| 4.4 - 4.8; yard = max |run - golden|; the goldens are stored as fp32):
    case  restatement - golden   fp32 yard (golden's own)   x3 yard   x3 yard, exact attention products
    a     1.2e-7                 1.58e-6                    3.17e-5   2.93e-5
    b     2.1e-7                 2.06e-6                    2.89e-5   2.87e-5
    c     2.3e-7                 3.52e-6                    3.32e-5   3.20e-5
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _whisper_enc_ref as R
from hirest_amd import _lib, synth, whisper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
ENC_SEED = 73                          # make_whisper_golden.py's


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_restatement_reproduces_the_goldens(case):
    """The unsplit restatement is the goldens' module (transformers' WhisperEncoder in fp64) to 4 x 2^-24 x max |ref|: the goldens are
    stored as fp32, half an ulp each.  The split run's distance from the golden is the x3 yard; it is printed, not asserted."""
    cfg, clips = synth.WHISPER_CASES[case]
    sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
    mel = synth.whisper_mel_input(cfg, clips, ENC_SEED)
    z = np.load(os.path.join(GOLDEN, f"whisper_enc_{case}.npz"))
    want = torch.from_numpy(z["out"]).double()
    got = R.encoder(cfg, sd, mel)
    peak = float(want.abs().max())
    err = float((got - want).abs().max())
    x3 = float((R.encoder(cfg, sd, mel, split=True) - want).abs().max())
    x3_exact_attn = float((R.encoder(cfg, sd, mel, split=True, split_attention=False) - want).abs().max())
    print(f"whisper encoder restatement {case}: - golden {err:.2e} (bar {4 * 2.0 ** -24 * peak:.2e}), max |ref| {peak:.2f}, fp32 yard "
          f"{float(z['yard']):.2e}, x3 yard {x3:.2e} ({x3 / float(z['yard']):.1f} x fp32's), with exact attention products {x3_exact_attn:.2e}")
    assert got.shape == want.shape and err <= 4 * 2.0 ** -24 * peak


def test_split_product_is_the_format():
    """hi + lo carries 16 significand bits and the three kept terms are exact in fp64: the split product misses a b by the lo x lo
    term and the two roundings of lo, about 2^-16 |a| |b| per term"""
    a = synth.tensor("x3host.a", (5, 64), 1.0, 3).double()
    b = synth.tensor("x3host.b", (64, 7), 1.0, 4).double()
    err = (R.product(a, b, True) - a @ b).abs().max().item()
    assert 0.0 < err <= 2.0 ** -15 * float((a.abs() @ b.abs()).max())
    assert torch.equal(R.product(a, b, False), a @ b)


def test_set_precision_on_the_cpu(monkeypatch):
    cfg = synth.WHISPER_TINY_A
    sd = synth.whisper_encoder_state_dict(cfg, ENC_SEED)
    enc = whisper.AudioEncoder(cfg, sd)
    assert enc.precision == "fp32" and whisper.AudioEncoder.PRECISIONS == ("fp32", "bf16x3")
    calls = []
    monkeypatch.setattr(enc, "prepared_weights", lambda: calls.append("fp32"))
    monkeypatch.setattr(enc, "prepared_weights_x3", lambda: calls.append("x3"))
    assert enc.set_precision("bf16x3") is enc and enc.precision == "bf16x3"            # prepares nothing, needs no GPU
    assert enc.set_precision("fp32").precision == "fp32"
    assert calls == [] and enc._cache is None and enc._cache_kinds == {}
    for bad in ("bf16", "fp16", "x3", "", None):
        with pytest.raises(ValueError):
            enc.set_precision(bad)
    assert enc.precision == "fp32"
    # the operand format's 32-column blocks: a width (or ffn) that is no multiple of 32 has no bf16x3 form
    odd = dict(cfg, d_model=144, encoder_attention_heads=2, encoder_ffn_dim=576)
    narrow = whisper.AudioEncoder(odd, synth.whisper_encoder_state_dict(odd, 5))
    with pytest.raises(NotImplementedError, match="144"):
        narrow.set_precision("bf16x3")
    assert narrow.set_precision("fp32").precision == "fp32"
    for width, heads in ((384, 6), (512, 8), (768, 12), (1024, 16), (1280, 20)):          # every released width passes
        c = dict(cfg, d_model=width, encoder_attention_heads=heads, encoder_ffn_dim=4 * width, encoder_layers=1, max_source_positions=3)
        assert whisper.AudioEncoder(c, synth.whisper_encoder_state_dict(c, 5)).set_precision("bf16x3").precision == "bf16x3"
    # no CPU fallback in this precision either
    with pytest.raises(RuntimeError, match="MI355X only"):
        enc.set_precision("bf16x3")(synth.whisper_mel_input(cfg, 1, ENC_SEED))
    # every kind of preparation is dropped together by a move / cast
    enc._cache, enc._cache_kinds = {"stale": None}, {"x3": {"stale": None}}
    enc.float()
    assert enc._cache is None and enc._cache_kinds == {} and enc.precision == "bf16x3"


def _model_checkpoint(path):
    cfg, _, seed, _ = synth.WHISPER_DEC_CASES["p"]
    m = whisper.Whisper(cfg, {**{"encoder." + k: v for k, v in synth.whisper_encoder_state_dict(cfg, 3).items()},
                              **synth.whisper_decoder_state_dict(cfg, seed)})
    state = {**{"encoder." + k.replace("/", "."): v.data for k, v in m.encoder._parameters.items()},
             **{"decoder." + k.replace("/", "."): v.data for k, v in m.decoder._parameters.items()}}
    torch.save({"dims": dict(m.dims), "model_state_dict": state}, path)
    return str(path)


def test_loaders_honour_the_keyword_and_the_environment(tmp_path, monkeypatch):
    path = _model_checkpoint(tmp_path / "tiny.pt")
    monkeypatch.delenv("HIREST_WHISPER_PRECISION", raising=False)
    assert whisper.load_encoder(path).precision == "fp32" and whisper.load_model(path).precision == "fp32"
    assert whisper.load_encoder(path, precision="bf16x3").precision == "bf16x3"
    model = whisper.load_model(path, precision="bf16x3")
    assert model.precision == model.encoder.precision == "bf16x3"
    assert model.set_precision("fp32") is model and model.encoder.precision == "fp32"
    with pytest.raises(ValueError):
        model.set_precision("fp16")
    monkeypatch.setenv("HIREST_WHISPER_PRECISION", "bf16x3")
    assert whisper.load_encoder(path).precision == "bf16x3" and whisper.load_model(path).precision == "bf16x3"
    assert whisper.load_encoder(path, precision="fp32").precision == "fp32"               # the keyword wins over the environment
    assert whisper.load_model(path, precision="fp32").precision == "fp32"
    monkeypatch.setenv("HIREST_WHISPER_PRECISION", "bf16")
    with pytest.raises(ValueError):                                                       # a bad name fails the load, not the first call
        whisper.load_encoder(path)
    with pytest.raises(ValueError):
        whisper.load_model(path)
    assert whisper.load_model(path, precision="bf16x3").precision == "bf16x3"
    with pytest.raises(ValueError):
        whisper.load_encoder(path, precision="fp16")
    monkeypatch.setenv("HIREST_WHISPER_PRECISION", "")
    assert whisper.load_encoder(path).precision == "fp32"
    assert whisper.DecodingOptions().fp16 is True and whisper.DecodingOptions(fp16=False).fp16 is False      # still accepted, still ignored


def test_entries_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    new = set(re.findall(r"\b(hirest_whisper_encoder_x3\w*)\s*\(", hdr))
    assert new == {"hirest_whisper_encoder_x3_workspace_bytes", "hirest_whisper_encoder_x3_gemm_args", "hirest_whisper_encoder_x3_forward"}
    lib = _lib.load()
    for name in new:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.hirest_abi_version() == 4 and "#define HIREST_ABI_VERSION 4" in text
    # the bindings lay the two structs out as the header does
    for struct, cls in (("hirest_whisper_layer_x3", _lib.WhisperLayerX3), ("hirest_whisper_encoder_x3", _lib.WhisperEncoderX3)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"[\s*](\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    assert C.sizeof(_lib.WhisperLayerX3) == 12 * 8 and C.sizeof(_lib.WhisperEncoderX3) == 8 + 6 * 4 + 4 + 4 + 3 * 8
    assert (_lib.WHISPER_X3_GELU_PASS, _lib.WHISPER_X3_AUTO_TILES) == (1, 2)
    assert "whisper_enc_x3.hip" in __import__("hirest_amd.build", fromlist=["SOURCES"]).SOURCES


def _desc(width, heads, ffn, ctx, flags=0):
    return _lib.WhisperEncoderX3(struct_size=C.sizeof(_lib.WhisperEncoderX3), layers=1, heads=heads, width=width, ffn=ffn, ctx=ctx,
                                 flags=flags, ln_eps=1e-5)


def _product(desc, B, which):
    """(the hirest_gemm_args the forward passes for product `which` at B windows, the kernel hirest_gemm_bf16 launches for them)"""
    lib = _lib.load()
    args = _lib.GemmArgs()
    _lib.check(lib.hirest_whisper_encoder_x3_gemm_args(C.byref(desc), B, which, C.byref(args)), "hirest_whisper_encoder_x3_gemm_args")
    buf = C.create_string_buffer(64)
    _lib.check(lib.hirest_gemm_dispatch_name(C.byref(args), buf, 64), "hirest_gemm_dispatch_name")
    return args, buf.value.decode()


def test_products_take_the_split_operand_family_at_every_row_count():
    """small.en's four products at one window (M = 1500) and at eight (M = 12000): each is a HIREST_GEMM_X3 call — there is no fp32
    kernel behind that flag to fall back to — on gemm_t128x3, the same family (one K order) at both row counts, which is what makes a
    window's bits independent of the batch.  The 192-row tile form differs from the 128-row one in the tile height only."""
    X3, T128 = 2, 4                                                   # HIREST_GEMM_X3, HIREST_GEMM_X3_T128
    lib = _lib.load()
    text = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    EPI_F32, EPI_RESID, EPI_GELU_SPLIT2 = (int(re.search(r"\b%s\s*=\s*(\d+)" % n, text).group(1))
                                           for n in ("HIREST_EPI_BIAS_F32", "HIREST_EPI_BIAS_RESID_F32", "HIREST_EPI_BIAS_GELU_SPLIT2"))
    assert (EPI_F32, EPI_RESID, EPI_GELU_SPLIT2) == (4, 3, 9)
    desc = _desc(768, 12, 3072, 1500)
    want = {0: (2304, 768, EPI_F32, 2304), 1: (768, 768, EPI_RESID, 768), 2: (3072, 768, EPI_GELU_SPLIT2, 6144), 3: (768, 3072, EPI_RESID, 768)}
    for B in (1, 8):
        for which, (N, K, epi, ldo) in want.items():
            a, name = _product(desc, B, which)
            assert (a.M, a.N, a.K, a.lda, a.ldw, a.ldo, a.epilogue, a.flags) == (1500 * B, N, 2 * K, 2 * K, 2 * K, ldo, epi, X3 | T128), (B, which)
            assert a.struct_size == C.sizeof(_lib.GemmArgs) and not a.aux0 and not a.aux1            # no split-K scratch: one K order
            assert re.fullmatch(r"gemm_t128x3<%d, [23]>" % epi, name), (B, which, name)
    # the measurement switches are per descriptor and change what they say, nothing else
    a, name = _product(_desc(768, 12, 3072, 1500, _lib.WHISPER_X3_GELU_PASS), 8, 2)
    assert (a.epilogue, a.ldo, a.flags) == (EPI_F32, 3072, X3 | T128) and name.startswith("gemm_t128x3<4,")
    a, name = _product(_desc(768, 12, 3072, 1500, _lib.WHISPER_X3_AUTO_TILES), 8, 2)
    assert (a.epilogue, a.flags) == (EPI_GELU_SPLIT2, X3) and name == "gemm_pp256x3<9>"
    a, name = _product(_desc(768, 12, 3072, 1500, _lib.WHISPER_X3_AUTO_TILES), 1, 1)
    assert name == "gemm_t128x3<3, 2>"
    # shapes without a bf16x3 form are refused by every entry, before any pointer is looked at
    for bad in (_desc(144, 2, 576, 33), _desc(128, 2, 520, 33), _desc(128, 1, 512, 33), _desc(128, 3, 512, 33)):
        assert lib.hirest_whisper_encoder_x3_workspace_bytes(C.byref(bad), 1) == 0
        assert lib.hirest_whisper_encoder_x3_gemm_args(C.byref(bad), 1, 0, C.byref(_lib.GemmArgs())) == -2
        assert lib.hirest_whisper_encoder_x3_forward(C.byref(bad), None, 1, None, None, 0, None) in (-1, -2)
    good = _desc(128, 2, 512, 33)
    M, D, F = 3 * 33, 128, 512
    need = lib.hirest_whisper_encoder_x3_workspace_bytes(C.byref(good), 3)
    exact = M * D * 4 + M * 2 * D * 2 + M * max(3 * D, F) * 4 + M * 2 * F * 2          # residual, split A, q | k | v, split hidden
    assert exact <= need <= exact + 4 * 256
    assert lib.hirest_whisper_encoder_x3_gemm_args(C.byref(good), 1, 4, C.byref(_lib.GemmArgs())) == -1
