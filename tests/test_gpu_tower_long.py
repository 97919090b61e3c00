"""The bf16 vision towers past 272 tokens (csrc/tower.hip -> hirest_attention_bf16_long): a seeded OpenAI-style tower with a 24 x 24 grid
(577 tokens, ViT-L/14@336px's length; input 48 px, patch 2, width 128, 2 heads of 64, 2 layers) against the oracle on the CPU, held to the
bars tests/test_gpu_parity.py holds the same tower to at 50 tokens; the pruned last block (q_rows = 1) of an EVA-style tower at that
length; and the 50-token tower, whose attention launches must still be the short entry's."""
import pytest
import torch

from hirest_amd import synth
from test_gpu_parity import COS_MIN, REL_MAX, cos_rows, rel

pytestmark = pytest.mark.gpu

LONG = dict(synth.OPENAI_VIT_TINY, image_resolution=48, vision_patch_size=2)        # (48 / 2)^2 + 1 = 577 tokens
SEED = 31


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def long_model(dev):
    from hirest_amd import clip
    sd = synth.openai_clip_state_dict(LONG, SEED)
    model = clip.build_model(sd).to(dev)
    assert model.visual.num_tokens == 577 and model.visual.precision == "bf16" and model.visual.heads == 2
    return model, sd


def _attention_records(fn):
    """(tag, B * H, N, dh) of every attention launch fn() makes (include/hirest_hip.h, hirest_prof_record)."""
    from hirest_amd import _lib
    lib = _lib.load()
    _lib.check(lib.hirest_profile_enable(1), "hirest_profile_enable")
    try:
        out = fn()
        rec = (_lib.ProfRecord * 512)()
        n = lib.hirest_profile_collect(rec, 512)
        assert 0 <= n < 512
    finally:
        lib.hirest_profile_enable(0)
    return out, [(r.tag, r.d0, r.d1, r.d2) for r in rec[:n] if r.kind == 1]


def test_openai_tower_at_577_tokens_vs_oracle(dev, long_model):
    """encode_image at the default precision runs (before the streaming attention it failed in block 0 with HIREST_E_SHAPE) and agrees with
    the oracle's CLIP vision tower; both heads, the vendored one (patch tokens) and the pip package's (CLS row).  The pip head is row 0 of
    the same all-token call, so it equals that row of a second call bit for bit."""
    from oracle import ref_cpu
    model, sd = long_model
    img = synth.frames("openai_long.img", (3, 3, 48, 48), SEED + 1)
    got, records = _attention_records(lambda: model.encode_image(img.to(dev)))
    assert got.shape == (3, 576, LONG["embed_dim"])
    assert records == [(2, 3 * 2, 577, 64)] * LONG["vision_layers"]                # every block took the streaming kernel
    ref = ref_cpu.openai_encode_image(sd, img, LONG)
    c, r = cos_rows(got.cpu().reshape(-1, LONG["embed_dim"]), ref.reshape(-1, LONG["embed_dim"])), rel(got.cpu(), ref)
    print(f"openai 577-token tower, patch tokens: min cosine {c:.6f}, max|diff|/max|ref| {r:.4f}")
    assert c >= COS_MIN and r <= REL_MAX
    model.visual.pip_head = True
    try:
        cls = model.encode_image(img.to(dev))
        again = model.encode_image(img.to(dev))
    finally:
        model.visual.pip_head = False
    assert cls.shape == (3, LONG["embed_dim"]) and torch.equal(cls, again)
    ref_cls = ref_cpu.openai_encode_image(sd, img, LONG, pip_head=True)
    c, r = cos_rows(cls.cpu(), ref_cls), rel(cls.cpu(), ref_cls)
    print(f"openai 577-token tower, CLS head: min cosine {c:.6f}, max|diff|/max|ref| {r:.4f}")
    assert c >= COS_MIN and r <= REL_MAX
    # a frame's embedding does not depend on the call it rides in
    model.visual.max_frames_per_call = 2
    try:
        assert torch.equal(model.encode_image(img.to(dev)), got)
    finally:
        model.visual.max_frames_per_call = 2048


def test_pruned_last_block_at_577_tokens_is_bit_identical(dev):
    """An EVA-style tower (CLS head) with 577 tokens and 64-wide heads, 64 frames: the folded-LayerNorm path, whose last block computes
    attention for query row 0 only (hirest_attention_bf16_long with q_rows = 1).  Its embeddings equal the unpruned run's bit for bit —
    the invariant the towers keep at 257 tokens — and meet the oracle within the parity bars."""
    from hirest_amd.eva_clip import VisionTower
    from oracle import ref_cpu
    cfg = {"embed_dim": 64, "vision_cfg": {"image_size": 48, "layers": 2, "width": 256, "head_width": 64, "mlp_ratio": 4.0, "patch_size": 2}}
    sd = synth.eva_clip_state_dict(cfg, SEED, towers=("visual",))
    v = cfg["vision_cfg"]
    tower = VisionTower(v["image_size"], v["patch_size"], v["width"], v["layers"], v["width"] // v["head_width"], v["mlp_ratio"], cfg["embed_dim"])
    tower.load_state_dict({k[len("visual."):]: t for k, t in sd.items()}, strict=True)
    tower = tower.to(dev).eval()
    assert tower.num_tokens == 577 and tower.precision == "bf16" and tower.prune_last_block and tower.fold_layernorm
    img = synth.frames("eva_long.img", (64, 3, 48, 48), SEED + 2)
    pruned, records = _attention_records(lambda: tower(img.to(dev)))
    assert tower.fold_fallbacks == 0
    assert records == [(2, 64 * 4, 577, 64)] * 2
    tower.prune_last_block = False
    try:
        full = tower(img.to(dev))
    finally:
        tower.prune_last_block = True
    assert torch.equal(pruned, full)
    ref = ref_cpu.eva_encode_image(sd, img[:4], cfg)
    c, r = cos_rows(pruned[:4].cpu(), ref), rel(pruned[:4].cpu(), ref)
    print(f"eva-style 577-token tower, 64 frames: min cosine {c:.6f}, max|diff|/max|ref| {r:.4f}")
    assert c >= COS_MIN and r <= REL_MAX


def test_short_sequences_stay_on_the_short_entry(dev):
    """The same tower at its usual 50 tokens: every attention launch is the short entry's (profile tag 0 = not causal, N = 50; the
    streaming kernel records tag 2), so the routing moved nothing below 273 tokens, and the result is what test_gpu_parity.py pins."""
    from hirest_amd import clip
    c = synth.OPENAI_VIT_TINY
    model = clip.build_model(synth.openai_clip_state_dict(c, SEED)).to(dev)
    img = synth.frames("openai_short.img", (3, 3, 224, 224), SEED + 3).to(dev)
    got, records = _attention_records(lambda: model.encode_image(img))
    assert records == [(0, 3 * 2, 50, 64)] * c["vision_layers"]
    assert torch.equal(model.encode_image(img), got)
    # the short entry on this tower's shape, next to the long entry on the same activation: same contract, and the tower used the former
    from hirest_amd import _lib, ops
    qkv = synth.tensor("short.qkv", (3 * 50, 3 * 128), 1.0, 5).to(torch.bfloat16).to(dev)
    short, long_ = torch.empty((150, 128), dtype=torch.bfloat16, device=dev), torch.empty((150, 128), dtype=torch.bfloat16, device=dev)
    ops.attention(qkv, short, 3, 50, 2, 64, False)
    _lib.check(_lib.load().hirest_attention_bf16_long(qkv.data_ptr(), long_.data_ptr(), 3, 50, 2, 64, 0.125, 0, ops.stream_ptr()), "long")
    # (each is within X.attention_bound = 2^-7 of the column maximum of the fp64 result)
    assert (short.float() - long_.float()).abs().max().item() <= 2.0 ** -6 * qkv[:, 256:].float().abs().max().item()
