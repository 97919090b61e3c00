"""numpy restatements for the Whisper decoder tests: the tail's rules (whisper/decoding.py's SuppressBlank, SuppressTokens and
ApplyTimestampRules as transformers states them), its counter-based generator and Gumbel-max pick, and the attention formulas — in the
precision the caller picks, so that the fp32 evaluation's own error against fp64 is the yardstick of the kernels."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
NEG = -np.inf


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_bits(seed: int, serial: int, R: int, V: int) -> np.ndarray:
    """the generator's 24 bits for rows 0 .. R - 1 and tokens 0 .. V - 1 -> uint32 [R, V]"""
    with np.errstate(over="ignore"):
        key = mix64(np.uint64((serial << 32) | seed) + G)
        ctr = (np.arange(R, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(V, dtype=np.uint64)[None, :]
        return (mix64(key + ctr + G) >> np.uint64(40)).astype(np.uint32)


def gumbel(bits: np.ndarray, dtype=np.float64) -> np.ndarray:
    u = (((bits >> 1).astype(dtype) + dtype(0.5)) * dtype(1.0 / 8388608.0)).astype(dtype)      # the top 23 bits: exact in fp32 too
    return -np.log(-np.log(u))


class Consts:
    def __init__(self, n_vocab, eot, no_speech, no_timestamps, timestamp_begin, max_initial_timestamp_index, blank, suppress=(),
                 suppress_blank=True, timestamp_rules=True, monotonic=True):
        self.n_vocab, self.eot, self.no_speech, self.no_timestamps, self.timestamp_begin = n_vocab, eot, no_speech, no_timestamps, timestamp_begin
        self.max_initial_timestamp_index, self.blank, self.suppress = max_initial_timestamp_index, blank, sorted(set(suppress))
        self.suppress_blank, self.timestamp_rules, self.monotonic = suppress_blank, timestamp_rules, monotonic


def suppressed_before_lse(c: Consts, seq, V: int) -> np.ndarray:
    """bool [V]: what the filters take out of a row whose sampled tokens so far are ``seq``, before the log-sum-exp rule"""
    s = np.zeros(V, dtype=bool)
    s[c.n_vocab:] = True
    if len(seq) == 0 and c.suppress_blank:
        if c.blank >= 0:
            s[c.blank] = True
            s[c.eot] = True
    s[c.suppress] = True
    if not c.timestamp_rules:
        return s
    tb = c.timestamp_begin
    s[c.no_timestamps] = True
    last_ts = len(seq) >= 1 and seq[-1] >= tb
    pen_ts = len(seq) < 2 or seq[-2] >= tb
    if last_ts:
        if pen_ts:
            s[tb:] = True
        else:
            s[:c.eot] = True
    stamps = [t for t in seq if t >= tb]
    if stamps and c.monotonic:
        s[tb:stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1] = True
    if len(seq) == 0:
        s[:tb] = True
        if c.max_initial_timestamp_index is not None and c.max_initial_timestamp_index >= 0:
            s[tb + c.max_initial_timestamp_index + 1:] = True
    return s


def tail_row(c: Consts, logits: np.ndarray, seq, dtype=np.float64, temperature=0.0, noise=None):
    """One row of the tail in ``dtype``: -> dict(suppressed bool [V], pick, logprob of the pick, no_speech_prob (first position), lse_gap =
    logsumexp(timestamps) - max(text) (None where the rule has nothing to compare), margin = the top-2 gap of what the pick maximises)."""
    x = logits.astype(dtype)
    V = x.shape[0]
    s = suppressed_before_lse(c, seq, V)
    tb = c.timestamp_begin
    out = {"no_speech_prob": None, "lse_gap": None}
    if len(seq) == 0 and c.no_speech >= 0:
        raw = x[:c.n_vocab]
        e = np.exp(raw - raw.max())
        out["no_speech_prob"] = e[c.no_speech] / e.sum()

    def lse(v):
        m = v.max()
        return m + np.log(np.exp(v - m).sum())
    if c.timestamp_rules:
        ts, text = x[tb:][~s[tb:]], x[:tb][~s[:tb]]
        if ts.size and text.size:
            out["lse_gap"] = lse(ts) - text.max()
            if out["lse_gap"] > 0:
                s[:tb] = True
        elif ts.size:
            s[:tb] = True
    out["suppressed"] = s
    if s.all():
        out.update(pick=c.eot, logprob=dtype(0.0), margin=np.inf)
        return out
    score = np.where(s, NEG, x / dtype(temperature) + noise.astype(dtype) if temperature > 0 else x)
    pick = int(np.argmax(score))
    top = np.sort(score[~s])[-2:]
    out.update(pick=pick, logprob=x[pick] - lse(x[~s]), margin=float(top[-1] - top[0]) if top.size > 1 else np.inf)
    return out


def advance(c: Consts, seq, pick):
    """the row's history after a pick (None: the row has ended)"""
    return None if pick == c.eot else list(seq) + [pick]


def grammar_ok(c: Consts, seq) -> bool:
    """Does a sampled sequence (eot excluded) obey the timestamp grammar?  It opens with a timestamp no later than the limit, timestamps
    come in pairs (a single one only as the very last token), and they do not decrease."""
    tb = c.timestamp_begin
    if not seq:
        return True
    if seq[0] < tb or (c.max_initial_timestamp_index is not None and c.max_initial_timestamp_index >= 0 and seq[0] > tb + c.max_initial_timestamp_index):
        return False
    if any(t == c.no_timestamps or t >= c.n_vocab for t in seq):
        return False
    runs, i = [], 0
    while i < len(seq):                                   # maximal runs of timestamp tokens: (start index, length)
        if seq[i] >= tb:
            j = i
            while j < len(seq) and seq[j] >= tb:
                j += 1
            runs.append((i, j - i))
            i = j
        else:
            i += 1
    for start, n in runs:
        at_start, at_end = start == 0, start + n == len(seq)
        if n > 2 or (at_start and n != 1 and not at_end):
            return False
        if n == 1 and not (at_start or at_end) and seq[start + 1] < c.eot:       # (a marker token >= eot may follow, if it is not suppressed)
            return False
    stamps = [t for t in seq if t >= tb]
    return all(a <= b for a, b in zip(stamps, stamps[1:])) if c.monotonic else True


def cross_attention(q, k, v, scale, dtype=np.float64):
    """softmax(q k^T scale) v per head: q [H, 64], k / v [Tk, H, 64] -> [H, 64], the textbook formula in ``dtype``"""
    q, k, v = q.astype(dtype), k.astype(dtype), v.astype(dtype)
    s = np.einsum("hd,thd->ht", q, k) * dtype(scale)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return np.einsum("ht,thd->hd", p, v) / p.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# which fp32 GEMM kernel each call of a decode step gets (tests/test_gpu_whisper_widths.py and its host-side twin)
# ---------------------------------------------------------------------------------------------------------------------------------

STEP_ROW_COUNTS = [1, 5, 16, 17, 32, 33, 47, 48, 80, 96, 256]        # around 16 / 32 / 48 rows, transcribe_many's 80, the limit of a call


def step_dispatch(R, D, I, Vp, **fields):
    """call of hirest_whisper_decode_step -> (status, name) of hirest_gemm_f32_dispatch_name for R rows of a decoder of width D, MLP
    width I and Vp LM-head columns: ``qkv``, ``cross_q``, ``fc1`` and ``head`` are ln_gemm's (the ``ln`` entry where it takes the fused
    form, else the plain product after hirest_layernorm; ``*_fused`` says which), ``self_out``, ``cross_out`` and ``fc2`` the plain
    product with a residual.  ``fields``: cus and the switches (default: the device's and the process's)."""
    import ctypes
    from hirest_amd import _lib

    def name(entry, M, N, K, **kw):
        buf = ctypes.create_string_buffer(64)
        status = _lib.load().hirest_gemm_f32_dispatch_name(ctypes.byref(_lib.GemmF32Query.make(entry, M, N, K, **fields, **kw)), buf, 64)
        return status, buf.value.decode() if status == 0 else ""

    out = {}
    for call, N in (("qkv", 3 * D), ("cross_q", D), ("fc1", I), ("head", Vp)):
        fused = R <= 256 and D % 256 == 0 and D <= 1024 and (N < 8192 or (D == 768 and R <= 32))      # ln_gemm() in csrc/whisper_dec.hip
        out[call] = name("ln", R, N, D) if fused else name("gemm", R, N, D)
        out[call + "_fused"] = fused
    out["self_out"] = out["cross_out"] = name("gemm", R, D, D, has_resid=1)
    out["fc2"] = name("gemm", R, D, I, has_resid=1)
    return out


def check_small_en_step_families(R, names):
    """the kernel families a step of R rows takes at small.en's width (768, MLP 3072, 8192 or more LM-head columns)"""
    ok = lambda call: names[call][0] == 0
    assert all(ok(c) for c in ("qkv", "cross_q", "fc1", "head", "self_out", "cross_out", "fc2")), names
    assert names["qkv_fused"] and names["cross_q_fused"] and names["fc1_fused"] and names["head_fused"] == (R <= 32), names
    assert names["cross_q"][1] == "m16ln<3,1,2>", names
    if R <= 32:
        assert names["qkv"][1] == names["fc1"][1] == "m16ln<3,1,2>", names
        assert names["self_out"][1] == names["fc2"][1] == "m16<1,1,8>", names
        assert names["head"][1].startswith("m16ln_stream<"), names
    else:
        assert all(names[c][1].startswith("rows<mt=") and ",ln" in names[c][1] for c in ("qkv", "fc1")), names
        assert names["self_out"][1] == "m16<2,1,6>" and names["fc2"][1] == "m16<1,1,4>", names
        head = names["head"][1]
        assert head in ("skinny", "tile64") or (head.startswith("rows<mt=") and ",ln" not in head), names
