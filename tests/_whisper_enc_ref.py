"""A torch fp64 restatement of the Whisper audio encoder, written from the definition ``AudioEncoder.forward`` documents (whisper/model.py):
conv1d k 3 + erf GELU, conv1d k 3 stride 2 + GELU, + positional embedding, pre-LN blocks (the key projection has no bias), ln_post, every
LayerNorm with eps 1e-5 and the biased variance.  Weights under WhisperEncoder's names (hirest_amd.synth.whisper_encoder_state_dict).

``split=True`` forms every Linear product — and, with ``split_attention``, both attention products — the way the bf16x3 kernels do:
``a_hi w_lo + a_lo w_hi + a_hi w_hi`` with ``hi = bf16(fp32(v))`` and ``lo = bf16(fp32(v) - hi)``, the three terms exact and summed in fp64.
Everything else stays fp64, so what the switch adds is the operand format's own error and nothing else: the yardstick of
tests/test_gpu_whisper_x3.py.  The stem is never split (it is exact fp32 on the device in both precisions).

tests/test_whisper_x3_host.py pins the unsplit restatement to tests/golden/whisper_enc_{a,b,c}.npz (transformers' WhisperEncoder in fp64)."""
import torch

F = torch.nn.functional
LN_EPS = 1e-5


def _hi_lo(v):
    v32 = v.float()
    hi = v32.to(torch.bfloat16)
    lo = (v32 - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def product(a, b, split):
    """a [..., M, K] @ b [..., K, N] in fp64; ``split``: from the bf16 hi + lo parts of both operands, without the lo x lo term"""
    if not split:
        return a @ b
    ah, al = _hi_lo(a)
    bh, bl = _hi_lo(b)
    return ah @ bl + al @ bh + ah @ bh


def _linear(x, w, b, split):
    y = product(x, w.double().t(), split)
    return y if b is None else y + b.double()


def _ln(x, sd, name):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"].double(), sd[name + ".bias"].double(), LN_EPS)


def stem(cfg, sd, mel):
    x = F.gelu(F.conv1d(mel.double(), sd["conv1.weight"].double(), sd["conv1.bias"].double(), padding=1))
    x = F.gelu(F.conv1d(x, sd["conv2.weight"].double(), sd["conv2.bias"].double(), stride=2, padding=1))
    return x.permute(0, 2, 1) + sd["embed_positions.weight"].double()


def attention_heads(q, k, v, split):
    """q [B, H, Tq, dh], k, v [B, H, Tk, dh] -> [B, H, Tq, dh]: softmax(q k^T dh^-0.5) v.  ``split``: the score product on the split of q
    and k, scaled afterwards; the second product on the split of exp(score - row max) and v, divided by the fp64 row sum afterwards (the
    flash kernel normalises at the end too).  Also the yardstick of tests/test_gpu_attention_x3_exact.py (_exact_inputs.attention_x3_restated)."""
    s = product(q, k.transpose(-1, -2), split) * q.shape[-1] ** -0.5
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return product(p, v, split) / p.sum(dim=-1, keepdim=True)


def attention(q, k, v, heads, split):
    """q, k, v [B, T, D] -> [B, T, D]: attention_heads per head."""
    B, T, D = q.shape
    dh = D // heads
    q, k, v = (t.reshape(B, T, heads, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    return attention_heads(q, k, v, split).permute(0, 2, 1, 3).reshape(B, T, D)


def encoder(cfg, sd, mel, split=False, split_attention=True):
    """mel [B, n_mels, 2 ctx] -> [B, ctx, width] fp64"""
    with torch.no_grad():
        x = stem(cfg, sd, mel)
        heads = cfg["encoder_attention_heads"]
        for i in range(cfg["encoder_layers"]):
            p = f"layers.{i}."
            h = _ln(x, sd, p + "self_attn_layer_norm")
            q = _linear(h, sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.q_proj.bias"], split)
            k = _linear(h, sd[p + "self_attn.k_proj.weight"], None, split)
            v = _linear(h, sd[p + "self_attn.v_proj.weight"], sd[p + "self_attn.v_proj.bias"], split)
            a = attention(q, k, v, heads, split and split_attention)
            x = x + _linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], split)
            h = _ln(x, sd, p + "final_layer_norm")
            h = F.gelu(_linear(h, sd[p + "fc1.weight"], sd[p + "fc1.bias"], split))
            x = x + _linear(h, sd[p + "fc2.weight"], sd[p + "fc2.bias"], split)
        return _ln(x, sd, "layer_norm")
