"""GPU parity: the HIP path, called through the C ABI (hirest_amd.ops / the tower runners),
against the CPU oracle and the reference's golden vectors.

Tolerances (stated, because the reference is fp32 and the MI355X path computes GEMMs/attention
in bf16 on MFMA with fp32 accumulation, fp32 residual stream / LayerNorm / softmax):
  * integer / index work (tokens, EOT index, top-k ranks with ties): bit-exact;
  * single kernels fed identical bf16-rounded operands: error bounded by the OUTPUT rounding
    (bf16 out: 2^-8 relative; f32 out: 1e-5 relative to the row scale);
  * whole towers vs the fp32 reference: cosine >= 0.999 per embedding row and
    max|diff| <= 3 % of max|ref| (bf16 operand rounding through up to 40 residual layers).
"""
import json
import os

import numpy as np
import pytest
import torch

from hirest_amd import synth

pytestmark = pytest.mark.gpu

COS_MIN = 0.999
REL_MAX = 0.03


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hirest_amd import ops as o
    return o


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def cos_rows(a, b):
    a, b = a.double(), b.double()
    return ((a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).min().item()


# ----------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------
@pytest.fixture(params=[1, 2, 3, 4, 5, 6, 7, 8, 9], ids=["t128", "t256x4", "t256x5", "t256p", "t256q", "p256w8", "p256w4", "pp256", "pq256"])
def gemm_kernel(request, ops):
    ops.gemm_select_kernel(request.param)
    yield request.param
    ops.gemm_select_kernel(0)


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 132, 128), (257, 1408, 1408), (1000, 4224, 1408), (77, 768, 3072),
                                   (513, 260, 64), (2056, 1408, 6144),
                                   (6151, 2100, 192), (6151, 1408, 192), (5000, 300, 64)])   # > 32 tiles per XCD, odd step count: persistent blocks walk several tiles
def test_gemm_epilogues(dev, ops, gemm_kernel, M, N, K):
    from hirest_amd import _lib
    a = synth.tensor("g.a", (M, K), 1.0, 7)
    w = synth.tensor("g.w", (N, K), 0.05, 7)
    bias = synth.tensor("g.b", (N,), 0.5, 7)
    ab, wb = a.to(torch.bfloat16), w.to(torch.bfloat16)
    ref = (ab.double() @ wb.double().t()) + bias.double()
    ad, wd, bd = ab.to(dev), wb.to(dev), bias.to(dev)
    scale = ref.abs().max().item()
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=dev)
    ops.gemm(ad, wd, bd, out, _lib.EPI_BIAS_BF16)
    assert (out.cpu().double() - ref).abs().max().item() <= scale * 2 ** -8
    ops.gemm(ad, wd, bd, out, _lib.EPI_BIAS_GELU_BF16)
    g = torch.nn.functional.gelu(ref)
    assert (out.cpu().double() - g).abs().max().item() <= scale * 2 ** -8
    ops.gemm(ad, wd, bd, out, _lib.EPI_BIAS_QGELU_BF16)
    qg = ref * torch.sigmoid(1.702 * ref)
    assert (out.cpu().double() - qg).abs().max().item() <= scale * 2 ** -8
    o32 = torch.empty((M, N), dtype=torch.float32, device=dev)
    ops.gemm(ad, wd, None, o32, _lib.EPI_BIAS_F32)
    assert (o32.cpu().double() - (ref - bias.double())).abs().max().item() <= scale * 1e-5
    resid = synth.tensor("g.r", (M, N), 1.0, 7)
    x = resid.to(dev).clone()
    ops.gemm(ad, wd, bd, x, _lib.EPI_BIAS_RESID_F32)
    assert (x.cpu().double() - (resid.double() + ref)).abs().max().item() <= scale * 1e-5


@pytest.mark.parametrize("order_bits", [8, 16, 32, 48])
def test_gemm_persistent_tile_orders(dev, ops, order_bits):
    """The persistent kernel's alternative tile walks (debug bits 3-5: grouped / panel-major / paired edge units) visit
    every tile exactly once: results equal the default order's."""
    from hirest_amd import _lib
    lib = _lib.load()
    ops.gemm_select_kernel(6)
    try:
        for (M, N, K) in [(6151, 1408, 192), (6151, 2100, 128), (4400, 4224, 64)]:
            a = synth.tensor("go.a", (M, K), 1.0, 9).to(torch.bfloat16).to(dev)
            w = synth.tensor("go.w", (N, K), 0.05, 9).to(torch.bfloat16).to(dev)
            bias = synth.tensor("go.b", (N,), 0.5, 9).to(dev)
            ref = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=dev)
            ops.gemm(a, w, bias, ref, _lib.EPI_BIAS_BF16)
            lib.hirest_gemm_debug_mode(order_bits)
            out = torch.full((M, N), 5.0, dtype=torch.bfloat16, device=dev)
            ops.gemm(a, w, bias, out, _lib.EPI_BIAS_BF16)
            lib.hirest_gemm_debug_mode(0)
            assert torch.equal(out, ref), (M, N, K, order_bits)
    finally:
        lib.hirest_gemm_debug_mode(0)
        ops.gemm_select_kernel(0)


def test_gemm_detects_transpose(dev, ops, gemm_kernel):
    """A = I against an asymmetric W: a swapped C layout cannot pass."""
    from hirest_amd import _lib
    n = 256
    a = torch.eye(n, dtype=torch.bfloat16, device=dev)
    w = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251 - 125).to(torch.bfloat16).to(dev)
    out = torch.empty((n, n), dtype=torch.float32, device=dev)
    ops.gemm(a, w, None, out, _lib.EPI_BIAS_F32)
    assert torch.equal(out, w.float().t())


def test_patch_embed_gemm(dev, ops):
    from hirest_amd import _lib
    from oracle import ref_cpu as O
    B, D, P = 3, 128, 14
    sd = {"visual.patch_embed.proj.weight": bf16_round(synth.tensor("pe.w", (D, 3, P, P), 0.05, 3)),
          "visual.patch_embed.proj.bias": synth.tensor("pe.b", (D,), 0.1, 3),
          "visual.cls_token": synth.tensor("pe.c", (1, 1, D), 0.1, 3),
          "visual.pos_embed": synth.tensor("pe.p", (1, 257, D), 0.1, 3)}
    img = bf16_round(synth.frames("pe.img", (B, 3, 224, 224), 3))
    ref = O.eva_patch_embed(sd, img, P)
    K, kpad = 3 * P * P, 640
    patches = torch.empty((B * 256, kpad), dtype=torch.bfloat16, device=dev)
    ops.patchify(img.to(dev), P, kpad, patches)
    # im2col is exact data movement
    want = img.reshape(B, 3, 16, P, 16, P).permute(0, 2, 4, 1, 3, 5).reshape(B * 256, K)
    assert torch.equal(patches[:, :K].float().cpu(), want) and patches[:, K:].float().abs().max().item() == 0
    pw = torch.zeros((D, kpad)); pw[:, :K] = sd["visual.patch_embed.proj.weight"].reshape(D, K)
    x = torch.zeros((B * 257, D), dtype=torch.float32, device=dev)
    pos = sd["visual.pos_embed"].reshape(257, D).contiguous().to(dev)
    ops.gemm(patches, pw.to(torch.bfloat16).to(dev), sd["visual.patch_embed.proj.bias"].to(dev), x, _lib.EPI_PATCH_POS_F32,
             pos=pos, patches_per_frame=256)
    ops.write_cls_rows(x, sd["visual.cls_token"].reshape(-1).to(dev), pos, B, 257, D)
    assert rel(x.cpu().reshape(B, 257, D), ref) < 1e-5


def test_patchify_uint8_fused_normalize(dev, ops):
    B, P, kpad = 2, 14, 640
    u = (synth.uniform_pm1("u8", B * 224 * 224 * 3, 1).reshape(B, 224, 224, 3) * 127 + 128).astype(np.uint8)
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]); std = torch.tensor([0.26862954, 0.26130258, 0.27577711])
    img = (torch.from_numpy(u).float().permute(0, 3, 1, 2) / 255.0 - mean[None, :, None, None]) / std[None, :, None, None]
    want = img.reshape(B, 3, 16, P, 16, P).permute(0, 2, 4, 1, 3, 5).reshape(B * 256, 588).to(torch.bfloat16)
    patches = torch.empty((B * 256, kpad), dtype=torch.bfloat16, device=dev)
    ops.patchify(torch.from_numpy(u).to(dev), P, kpad, patches, mean.to(dev), std.to(dev))
    # bit equality: with CLIP's mean / std every one of the 256 x 3 values lies more than ten fp32 error bounds away from a bf16 rounding
    # midpoint, so no fp32 evaluation order changes the bf16 result (derived in test_gpu_tower_kernels.py::test_patchify_uint8_exhaustive_bit_exact)
    assert torch.equal(patches[:, :588].cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("rows,D,eps", [(257 * 2, 1408, 1e-6), (77, 768, 1e-5), (10, 512, 1e-12), (5, 384, 1e-5), (9, 6144, 1e-5),
                                          (8227, 1408, 1e-6), (9001, 768, 1e-5)])
def test_layernorm(dev, ops, rows, D, eps):
    from oracle import ref_cpu as O
    x = synth.tensor("ln.x", (rows, D), 2.0, 5, mean=0.3)
    g = synth.tensor("ln.g", (D,), 0.2, 5, mean=1.0)
    b = synth.tensor("ln.b", (D,), 0.2, 5)
    ref = O.layer_norm(x.double(), g.double(), b.double(), eps)
    o32 = torch.empty((rows, D), dtype=torch.float32, device=dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), eps, o32)
    assert (o32.cpu().double() - ref).abs().max().item() < 2e-5
    o16 = torch.empty((rows, D), dtype=torch.bfloat16, device=dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), eps, o16)
    assert (o16.cpu().double() - ref).abs().max().item() <= ref.abs().max().item() * 2 ** -8
    idx = torch.tensor([rows - 1, 0, rows // 2], dtype=torch.int32)
    og = torch.empty((3, D), dtype=torch.float32, device=dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), eps, og, row_index=idx.to(dev))
    assert torch.equal(og.cpu(), o32.cpu()[idx.long()])


def _attention_ref(qkv, B, N, H, dh, causal):
    D = H * dh
    q, k, v = qkv.double().reshape(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    if causal:
        s = s + torch.full((N, N), float("-inf"), dtype=torch.float64).triu_(1)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, D)


@pytest.mark.parametrize("B,N,H,dh,causal,qscale", [(2, 257, 16, 88, False, 1.0), (3, 77, 12, 64, True, 1.0),
                                                    (1, 257, 8, 88, False, 6.0), (2, 50, 12, 64, False, 1.0),
                                                    (1, 1, 2, 64, True, 1.0), (1, 272, 2, 64, False, 3.0),
                                                    (70, 257, 16, 88, False, 2.0), (66, 200, 4, 64, True, 1.0)])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7], ids=["v1", "v2", "v3", "v3w12", "v3lean", "v3leanprod", "v3prod"])
def test_attention(dev, ops, B, N, H, dh, causal, qscale, variant):
    ops.attention_select_kernel(variant)
    D = H * dh
    qkv = bf16_round(synth.tensor(f"at.{N}.{dh}", (B * N, 3 * D), 1.0, 9))
    qkv[:, :D] *= qscale   # peaky softmax when qscale > 1
    qkv = bf16_round(qkv)
    ref = _attention_ref(qkv, B, N, H, dh, causal)
    out = torch.full((B * N, D), 9.0, dtype=torch.bfloat16, device=dev)
    ops.attention(qkv.to(torch.bfloat16).to(dev), out, B, N, H, dh, causal)
    ops.attention_select_kernel(ops.ATTENTION_DEFAULT_KERNEL)
    # P is rounded to bf16 before P.V and the output is bf16: 2 roundings of <= 2^-8 relative to max|v|
    assert (out.cpu().double() - ref).abs().max().item() <= 3 * 2 ** -8 * qkv[:, 2 * D:].abs().max().item()


@pytest.mark.parametrize("B,N,H,dh,q_rows", [(70, 257, 16, 88, 257), (128, 257, 16, 88, 1), (300, 100, 4, 64, 100), (97, 257, 8, 88, 33)])
@pytest.mark.parametrize("variant", [3, 5, 6, 7], ids=["v3", "v3lean", "v3leanprod", "v3prod-default"])
def test_attention_by_head_mapping_is_bit_identical(dev, ops, B, N, H, dh, q_rows, variant):
    """hirest_attention_set_mapping: one head per workgroup over frames == one frame per workgroup over heads (default), for batch
    sizes that leave some workgroups a step short, and for the leading-rows form."""
    from hirest_amd import _lib
    D = H * dh
    g = torch.Generator(device="cpu"); g.manual_seed(B + N)
    qkv = torch.randn((B * N, 3 * D), generator=g).to(torch.bfloat16).to(dev)
    outs = []
    ops.attention_select_kernel(variant)
    try:
        for by_head in (False, True):
            ops.attention_set_mapping(by_head)
            out = torch.full((B * N, D), 9.0, dtype=torch.bfloat16, device=dev)
            _lib.check(_lib.load().hirest_attention_bf16_rows(qkv.data_ptr(), out.data_ptr(), B, N, H, dh, dh ** -0.5, 0, q_rows,
                                                              torch.cuda.current_stream().cuda_stream), "hirest_attention_bf16_rows")
            outs.append(out.reshape(B, N, D)[:, :q_rows].clone())
    finally:
        ops.attention_select_kernel(ops.ATTENTION_DEFAULT_KERNEL)
        ops.attention_set_mapping(None)                 # back to automatic (by head below 256 frames)
    assert torch.equal(outs[0], outs[1])
    assert bool(torch.isfinite(outs[1].float()).all()) and float(outs[1].float().abs().max()) < 9.0


def test_embed_tokens_exact(dev, ops):
    B, L, D, V = 5, 77, 128, 49408
    tok = synth.tokens("emb.tok", B, 4)
    emb = synth.tensor("emb.w", (V, D), 0.02, 4)
    pos = synth.tensor("emb.p", (L, D), 0.01, 4)
    x = torch.empty((B * L, D), dtype=torch.float32, device=dev)
    eot = torch.empty((B,), dtype=torch.int32, device=dev)
    ops.embed_tokens(tok.to(dev), emb.to(dev), pos.to(dev), x, eot)
    assert torch.equal(x.cpu().reshape(B, L, D), emb[tok] + pos)
    assert torch.equal(eot.cpu().long(), torch.arange(B) * L + tok.argmax(-1))


@pytest.mark.parametrize("Q,V,k", [(5, 152620, 5), (3, 91572, 3), (7, 16384, 10), (2, 20001, 16)])
def test_topk_long_rows_two_pass(dev, ops, Q, V, k):
    """Chunked two-pass selection (beam search over beams*vocab) == the single-pass kernel == the oracle, ties included."""
    from oracle import ref_cpu as O
    from hirest_amd import _lib
    s = synth.tensor("tk.long", (Q, V), 1.0, 5)
    s = (s * 64).round() / 64                       # few distinct values: many exact ties
    tie = torch.from_numpy(np.random.default_rng(1).permutation(V).astype(np.int32))
    sd = s.to(dev)
    for tr in (None, tie):
        trd = None if tr is None else tr.to(dev)
        val, idx = ops.topk(sd, k, trd)
        ref = O.topk_with_ties(s, tr if tr is not None else torch.arange(V, dtype=torch.int32), k)
        assert torch.equal(idx.cpu().long(), ref.long())
        assert torch.equal(val.cpu(), torch.gather(s, 1, ref.long()))
        i1 = torch.empty((Q, k), dtype=torch.int32, device=dev)         # single-pass kernel through the plain entry point
        _lib.check(_lib.load().hirest_topk_f32(sd.data_ptr(), None if trd is None else trd.data_ptr(), Q, V, k,
                                              i1.data_ptr(), None, ops.stream_ptr()), "topk")
        assert torch.equal(i1, idx)


def test_pool_similarity_topk(dev, ops, golden_dir):
    from oracle import ref_cpu as O
    V, F, E, Q = 37, 32, 1024, 19
    fe = synth.tensor("pool.fe", (V, F, E), 1.0, 8, mean=0.1)
    for nf in (False, True):
        got = ops.pool_l2norm(fe.to(dev), nf).cpu()
        assert (got - O.pool_video(fe, nf)).abs().max().item() < 2e-6
    te = O.l2_normalize(synth.tensor("pool.te", (Q, E), 1.0, 8))
    vn = O.pool_video(fe)
    s = ops.similarity(te.to(dev), vn.to(dev)).cpu()
    assert (s - O.similarity(te, vn)).abs().max().item() < 1e-5
    # ranking with deliberate exact ties, reference tie rule (evaluate.py:58-60)
    d = json.load(open(os.path.join(golden_dir, "retrieval_eval.json")))
    names, prompts = d["names"], d["prompts"]
    u = synth.uniform_pm1("eval.scores", len(prompts) * len(names), d["scores_seed"]).reshape(len(prompts), -1)
    scores = torch.from_numpy(np.round(u * 8).astype(np.float32) / 8.0)
    order = sorted(range(len(names)), key=lambda i: names[i])
    tie = torch.empty(len(names), dtype=torch.int32)
    tie[torch.tensor(order)] = torch.arange(len(names), dtype=torch.int32)
    val, idx = ops.topk(scores.to(dev), 50, tie.to(dev))
    want = O.topk_with_ties(scores, tie.long(), 50)
    assert torch.equal(idx.cpu().long(), want)
    for q in range(len(prompts)):
        assert [names[i] for i in idx[q, :10].tolist()] == d["ranked_top10"][q]
    assert torch.equal(val.cpu(), torch.gather(scores, 1, want))


# ----------------------------------------------------------------------------------------
# towers vs the reference's golden vectors
# ----------------------------------------------------------------------------------------
def _check_embed(got, ref, what):
    c, r = cos_rows(got, ref), rel(got, ref)
    print(f"{what}: min cosine {c:.6f}, max|diff|/max|ref| {r:.4f}")
    assert c >= COS_MIN and r <= REL_MAX


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_eva_tiny_towers_vs_reference(dev, golden_dir, precision):
    import hirest_amd
    g = np.load(os.path.join(golden_dir, "eva_tiny.npz"))
    seed = int(g["seed"])
    model, _ = hirest_amd.build_eva_model_and_transforms("EVA_CLIP_tiny_test", pretrained=f"synth:{seed}", precision=precision)
    model = model.to(dev).eval()
    assert model.visual.precision == model.text.precision == precision
    img = synth.frames("eva_tiny.img", (int(g["n_img"]), 3, 224, 224), seed + 1).to(dev)
    tok = torch.from_numpy(g["tokens"]).to(dev)
    _check_embed(model.encode_image(img).cpu(), torch.from_numpy(g["image_embed"]), "tiny image")
    _check_embed(model.encode_text(tok).cpu(), torch.from_numpy(g["text_embed"]), "tiny text")
    fi, ft, ls = model(img, tok)
    _check_embed(fi.cpu(), torch.from_numpy(g["fwd_image"]), "tiny fwd image")
    _check_embed(ft.cpu(), torch.from_numpy(g["fwd_text"]), "tiny fwd text")
    assert abs(ls.item() - float(g["logit_scale_exp"])) < 1e-4
    assert torch.equal(model(None, tok), model.encode_text(tok))
    if precision == "fp32":   # the reference-precision towers (csrc/tower_f32.hip): fp32 agreement, not the bf16 bar
        for got, key in ((model.encode_image(img), "image_embed"), (model.encode_text(tok), "text_embed")):
            ref = torch.from_numpy(g[key])
            assert (got.cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), key
    # empty batches (the reference's modules return empty [0, E] tensors) and the reference's input checks
    assert tuple(model.encode_image(img[:0]).shape) == (0, fi.shape[1]) and tuple(model.encode_text(tok[:0]).shape) == (0, ft.shape[1])
    with pytest.raises(AssertionError):
        model.encode_image(img[:, :, :200, :200].contiguous())           # vit_model.py:203
    with pytest.raises(RuntimeError):
        model.encode_image(img.cpu())                                    # no CPU fallback


def test_eva_g14_full_size_vs_reference(dev, golden_dir):
    import hirest_amd
    g = np.load(os.path.join(golden_dir, "eva_g14.npz"))
    seed = int(g["seed"])
    model, _ = hirest_amd.build_eva_model_and_transforms("EVA_CLIP_g_14", pretrained=f"synth:{seed}")   # default = the reference's: fp32
    model = model.to(dev).eval()
    img = synth.frames("eva_g14.img", (int(g["n_img"]), 3, 224, 224), seed + 1).to(dev)
    tok = torch.from_numpy(g["tokens"]).to(dev)
    # ---- precision='fp32' (eva_clip.py:90 default): 40 exact-fp32 layers agree with the reference's fp32 outputs to ~1e-5, and a
    # row does not depend on what else is in the call
    assert model.visual.precision == "fp32"
    for got, key in ((model.encode_image(img), "image_embed"), (model.encode_text(tok), "text_embed")):
        ref = torch.from_numpy(g[key])
        err = (got.cpu() - ref).abs().max().item() / ref.abs().max().item()
        print(f"EVA-g/14 fp32 towers vs reference {key}: max |diff| / max |ref| = {err:.2e}")
        assert err <= 5e-5, (key, err)
    assert torch.equal(model.encode_image(torch.cat([img.flip(0), img], 0))[2:], model.encode_image(img))
    # ---- the bf16 MFMA towers (the measured hot path) from here on
    model.set_precision("bf16")
    out = model.encode_image(img)
    _check_embed(out.cpu(), torch.from_numpy(g["image_embed"]), "EVA-g/14 image (40 layers)")
    _check_embed(model.encode_text(tok).cpu(), torch.from_numpy(g["text_embed"]), "EVA-g/14 text (12 layers)")
    # size-independent properties: rows are independent => batching / chunking / order are bit-exact no-ops
    big = torch.cat([img, img.flip(0), img], 0)
    model.visual.max_frames_per_call = 4
    ob = model.encode_image(big)
    assert torch.equal(ob[:2], out) and torch.equal(ob[2:4], out.flip(0)) and torch.equal(ob[4:], out)
    model.visual.max_frames_per_call = 256
    assert torch.equal(model.encode_image(img[:1]), out[:1])
    # bf16 NCHW input = same result as f32 input holding bf16-representable values
    imb = img.to(torch.bfloat16)
    assert torch.equal(model.encode_image(imb), model.encode_image(imb.float()))
    # BASELINE configs[1] at full size: one 1024-frame tower call (persistent p256 / pp256 GEMMs, 263168-row activations)
    # with the golden frames planted among random ones; duplicates agree and chunking the big batch changes nothing
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    full = torch.randn((1024, 3, 224, 224), device=dev, generator=gen)
    spots = [0, 517, 1023]
    full[spots[0]], full[spots[1]], full[spots[2]] = img[0], img[1], img[0]
    model.visual.max_frames_per_call = 1024
    of = model.encode_image(full)
    assert torch.isfinite(of).all() and torch.equal(of[0], of[1023])
    # the reference's own outputs, now checked on rows of the full-size batch
    _check_embed(of[spots[:2]].cpu(), torch.from_numpy(g["image_embed"]), "EVA-g/14 image, rows of a 1024-frame call")
    # micro-batches of >= 64 frames all take the same kernels (below that the attention switches from the persistent
    # per-frame form to one workgroup per head, equal within rounding only): a 64-frame call reproduces the rows exactly
    assert torch.equal(model.encode_image(full[453:517 + 1])[-1], of[517])
    assert (of[spots[:2]] - out).abs().max().item() < 2e-2 * out.abs().max().item()
    model.visual.max_frames_per_call = 384                      # 384 + 384 + 256: ragged micro-batches
    assert torch.equal(model.encode_image(full), of)
    # a call twice the bench size (activations past 2^32 bytes: 64-bit addressing everywhere) reproduces the same rows
    model.visual.max_frames_per_call = 2048
    assert torch.equal(model.encode_image(torch.cat([full, full.flip(0)], 0)), torch.cat([of, of.flip(0)], 0))
    # calls of >= 64 frames fold both LayerNorms of a block into its GEMMs (HIREST_EPI_LNFOLD_*); the plain path
    # (LayerNorm kernel + plain epilogues) on the same batch agrees within the bf16 rounding of the LayerNorm output
    # and meets the same bar against the reference's outputs; both are deterministic
    assert torch.equal(model.encode_image(full[:128]), of[:128])
    model.visual.fold_layernorm, model.visual._prepared = False, None
    plain = model.encode_image(full[:128])
    model.visual.fold_layernorm, model.visual._prepared = True, None
    _check_embed(plain[:1].cpu(), torch.from_numpy(g["image_embed"])[:1], "EVA-g/14 image, LayerNorm passes not folded")
    cos = torch.nn.functional.cosine_similarity(plain, of[:128], dim=1).min().item()
    print(f"folded vs plain LayerNorm path, 128 frames: min cosine {cos:.6f}")
    assert cos > 0.9998
    model.visual.max_frames_per_call = 256


# ----------------------------------------------------------------------------------------
# OpenAI-CLIP ViT as vendored by the reference (EVA_clip/model.py) — BASELINE configs[0] on the GPU
# ----------------------------------------------------------------------------------------
def test_openai_clip_tiny_vs_reference(dev, golden_dir):
    from hirest_amd import clip
    g = np.load(os.path.join(golden_dir, "openai_tiny.npz"))
    c, seed = synth.OPENAI_VIT_TINY, int(g["seed"])
    sd = synth.openai_clip_state_dict(c, seed)
    model = clip.build_model(sd).to(dev)
    assert set(model.state_dict().keys()) == set(sd.keys())
    img = synth.frames("openai_tiny.img", (int(g["n_img"]), 3, 224, 224), seed + 1).to(dev)
    pt = model.encode_image(img)
    assert pt.shape == (int(g["n_img"]), 49, c["embed_dim"])          # patch tokens, CLS dropped (hazard H4)
    _check_embed(pt.reshape(-1, c["embed_dim"]).cpu(), torch.from_numpy(g["patch_tokens_sample"]).reshape(-1, c["embed_dim"]), "openai tiny patch tokens")
    _check_embed(model.encode_text(torch.from_numpy(g["tokens"]).to(dev)).cpu(), torch.from_numpy(g["text_embed"]), "openai tiny text")


def test_openai_clip_pip_head_vs_oracle(dev):
    """The pip `clip` package's CLS head (`clip.load(..., pip_head=True)`; inference_video_retrieval.py:169's model): PARITY UNPINNED —
    that package is not in the reference tree, so the yardstick is the oracle's restatement of its published forward
    (oracle/ref_cpu.py:openai_encode_image(pip_head=True)), whose tower is the one the vendored-head goldens pin."""
    from hirest_amd import clip
    from oracle import ref_cpu
    c, seed = synth.OPENAI_VIT_TINY, 23
    sd = synth.openai_clip_state_dict(c, seed)
    model = clip.build_model(sd).to(dev)
    img = synth.frames("openai_pip.img", (6, 3, 224, 224), seed + 1)
    model.visual.pip_head = True
    got = model.encode_image(img.to(dev))
    assert got.shape == (6, c["embed_dim"])
    _check_embed(got.cpu(), ref_cpu.openai_encode_image(sd, img, c, pip_head=True), "openai tiny CLS head (pip clip)")
    model.visual.pip_head = False
    assert model.encode_image(img.to(dev)).shape == (6, 49, c["embed_dim"])


def test_openai_clip_b32_config1_vs_reference(dev, golden_dir):
    """ViT-B/32, 64 frames + 16 real prompts: frame embedding = mean of projected patch tokens, cosine top-5."""
    from hirest_amd import clip
    g = np.load(os.path.join(golden_dir, "openai_b32.npz"))
    c, seed = synth.OPENAI_VIT_B32, int(g["seed"])
    model = clip.build_model(synth.openai_clip_state_dict(c, seed)).to(dev)
    img = synth.frames("openai_b32.img", (int(g["n_img"]), 3, 224, 224), seed + 1).to(dev)
    fe = model.encode_image(img).mean(dim=1)
    te = model.encode_text(torch.from_numpy(g["tokens"]).to(dev))
    _check_embed(fe.cpu(), torch.from_numpy(g["frame_embed"]), "ViT-B/32 frame embed")
    _check_embed(te.cpu(), torch.from_numpy(g["text_embed"]), "ViT-B/32 text embed")
    from hirest_amd import ops as o
    cos = o.similarity(o.pool_l2norm(te.unsqueeze(1).contiguous()), o.pool_l2norm(fe.unsqueeze(1).contiguous())).cpu()
    ref = torch.from_numpy(g["cosine"])
    err = (cos - ref).abs().max().item()
    print(f"config 1 cosine matrix: max |diff| {err:.2e}")
    assert err < 2e-2
    # top-5 ids: exact wherever the reference's margins exceed the bf16 score error
    r5 = ref.topk(6, dim=1).values
    safe = (r5[:, :5] - r5[:, 1:6]).min(dim=1).values > 2 * err
    got = cos.topk(5, dim=1).indices
    assert torch.equal(got[safe], torch.from_numpy(g["top5"])[safe])
    print(f"top-5 ids exact on {int(safe.sum())}/{len(safe)} queries with safe margins; "
          f"overall set agreement {np.mean([len(set(a.tolist()) & set(b.tolist())) / 5 for a, b in zip(got, torch.from_numpy(g['top5']))]):.3f}")
    # precision='fp32' (the reference's own arithmetic on the exact-fp32 kernels): SURVEY 8d C1's bar — ALL 16 top-5 lists equal the
    # reference's, cosines within 1e-5
    model.set_precision("fp32")
    fe32 = model.encode_image(img).mean(dim=1)
    te32 = model.encode_text(torch.from_numpy(g["tokens"]).to(dev))
    cos32 = o.similarity(o.pool_l2norm(te32.unsqueeze(1).contiguous()), o.pool_l2norm(fe32.unsqueeze(1).contiguous())).cpu()
    err32 = (cos32 - ref).abs().max().item()
    print(f"config 1 at precision fp32: max |cosine diff| {err32:.2e}")
    assert err32 <= 1e-5
    assert torch.equal(cos32.topk(5, dim=1).indices, torch.from_numpy(g["top5"]))
    assert (fe32.cpu() - torch.from_numpy(g["frame_embed"])).abs().max().item() <= 5e-5 * torch.from_numpy(g["frame_embed"]).abs().max().item()
    model.set_precision("bf16")
    assert torch.equal(model.encode_image(img).mean(dim=1), fe)                 # switching back rebuilds the bf16 descriptor: same bits
    with pytest.raises(ValueError):
        model.set_precision("int8")
