"""The search of step captioning (modeling.py:556-632 behind trim_feats and the encoder): beam search over the 2-layer decoder.

One state object, ``BeamSearch``, owns the buffers of a search and issues its word steps; two short drivers use it — ``beam_search``
(eager: fresh buffers per call) and ``graph_beam_search`` (static buffers, the word steps replayed from hipGraphs) — next to the
full-prefix recompute the reference does (``full_prefix_search``) and ``caption_batches`` (several searches in flight)."""
import ctypes as C
import threading
import weakref
from itertools import accumulate
from types import SimpleNamespace
from typing import List

import torch

from . import _lib, ops
from .beam import BOS_ID, EOS_ID, BeamState


def beam_layout(B: int, num_beams: int, max_words: int) -> SimpleNamespace:
    """The device-side beam state (beam.py: scores, next_ys, prev_ks) and the inputs of the next step, in two packed buffers (one fill,
    two small copies and one read-back per batch instead of a dozen): name -> slice for int32 `ibuf` and float32 `fbuf`, their lengths,
    `readout` = everything the host read-out copies, `reset` = everything reset() re-initialises from the constants.  The ONLY place
    that knows an offset into either buffer."""
    R, nt = B * num_beams, B * max_words * num_beams

    def pack(**sizes):
        return {k: slice(e - n, e) for (k, n), e in zip(sizes.items(), accumulate(sizes.values()))}
    ibuf, fbuf = pack(tokens=nt, backptr=nt, n_steps=B, done=B, ids=R, parents=R), pack(add=R, scores=R)
    return SimpleNamespace(ibuf=ibuf, ibuf_len=ibuf["parents"].stop, fbuf=fbuf, fbuf_len=fbuf["scores"].stop,
                           readout=slice(0, ibuf["done"].start), reset=slice(ibuf["ids"].start, ibuf["parents"].stop))


def fused_tail_applies(model, num_beams: int, vocab_padded: int) -> bool:
    """hirest_caption_beam_step (the decoder step + log-softmax, top-k and beam bookkeeping in two kernels) within the tail kernels' limits."""
    return bool(getattr(model, "caption_fused_tail", True)) and num_beams <= 16 and vocab_padded <= 32768


class BeamSearch:
    """Buffers and word steps of one beam search without a host round trip per word: one C-side decoder step (csrc/caption.hip: ~35
    kernels enqueued without returning to Python, each beam's self-attention K / V kept and re-gathered by parent beam), the top-k over
    beams x vocabulary and the beam bookkeeping (`hirest_beam_advance`: beam.py:70-92) all stay on the device.  The host only watches
    the "done" flags to stop early.  The row set never shrinks: a finished sample's rows keep being computed and are ignored.

    static=False: the buffers of ONE call; the encoder K / V handed to load_encoder are adopted as they are.  static=True: buffers that
    captured graphs point into — load_encoder copies into them and reset() starts the next search."""

    def __init__(self, model, B, num_beams, max_words, F, nl, static: bool):
        c, lib = model._w(), _lib.load()
        dev = c["dev"]
        self.model, self.lib, self.static = weakref.proxy(model), lib, static      # (no cycle through the weight cache, which keeps the static searches)
        self.B, self.num_beams, self.max_words, self.F = B, num_beams, max_words, F
        self.desc = desc = model._dec_desc()                 # (a captured graph holds the descriptor of its precision)
        R, Dm, Vp = B * num_beams, 768, desc.vocab_padded
        self.Vp, self.fused_tail = Vp, fused_tail_applies(model, num_beams, Vp)
        if static:                                           # (caption_batches captures only where the fused tail applies)
            self._adopt([torch.empty((R, F, 2 * Dm), dtype=torch.float32, device=dev) for _ in range(nl)])
        self.cache = [torch.empty((2 * nl, R, max_words, Dm), dtype=torch.float32, device=dev) for _ in range(2)]   # ping-pong
        self.ptrs = [(C.c_void_p * (2 * nl))(*[cb[i].data_ptr() for i in range(2 * nl)]) for cb in self.cache]
        self.layout = L = beam_layout(B, num_beams, max_words)
        self.ibuf = torch.empty((L.ibuf_len,), dtype=torch.int32, device=dev)
        self.fbuf = torch.empty((L.fbuf_len,), dtype=torch.float32, device=dev)
        u8 = lambda n: torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
        t = {k: self.ibuf[s] for k, s in L.ibuf.items()}
        t.update({k: self.fbuf[s] for k, s in L.fbuf.items()}, logp=torch.empty((R, Vp), dtype=torch.float32, device=dev),
                 ws=u8(lib.hirest_caption_step_workspace_bytes(C.byref(desc), R)))
        if self.fused_tail:
            t["tail_ws"] = u8(lib.hirest_caption_beam_tail_workspace_bytes(B, num_beams, Vp))
        else:                                                # scratch of the separate top-k and the events behind the copies of the flags
            t.update(tk_ws=u8(lib.hirest_topk_workspace_bytes(B, num_beams * Vp, num_beams)),
                     val=torch.empty((B, num_beams), dtype=torch.float32, device=dev), idx=torch.empty((B, num_beams), dtype=torch.int32, device=dev))
            self.copied = {}
        # the tensors by name and their addresses, so that a word step is the C call and nothing else
        self.buf, self.ptr = SimpleNamespace(**t), SimpleNamespace(**{k: v.data_ptr() for k, v in t.items()})
        # the stamped done flags of every step, pinned.  The eager path takes ONE TABLE PER CALL: a table cached per shape could still be
        # written by kernels of an earlier call that left its loop by an exception, or by a concurrent call of the same shape on another
        # stream (caption_batches), and a stale stamp would end this search early
        self.done_rows = torch.zeros((max_words, B), dtype=torch.int32).pin_memory()
        self.done_host = [self.done_rows[w] for w in range(max_words)]
        self.done_ptrs = [d.data_ptr() for d in self.done_host]
        # constants of the search, built once per shape; they live in the weight cache
        key = ("beam_consts", B, num_beams, str(dev))
        if key not in c:
            add0 = torch.full((B, num_beams), -3.0e38, dtype=torch.float32)    # first step: only beam 0 competes
            add0[:, 0] = 0.0                                                   # (beam.py:78)
            c[key] = (torch.cat([torch.full((R,), BOS_ID, dtype=torch.int32), torch.arange(R, dtype=torch.int32)]).to(dev),
                      torch.cat([add0.reshape(-1), torch.zeros(R)]).to(dev))
        self.ibuf0, self.fbuf0 = c[key]
        self.graphs = []                                     # static: (first word, last word, hipGraph) per captured chunk

    def _adopt(self, enc):
        self.enc, self.enc_ptrs = enc, (C.c_void_p * len(enc))(*[e.data_ptr() for e in enc])

    def load_encoder(self, enc_kv_all: List[torch.Tensor]):
        """The encoder-side K / V of the cross-attention, one row set per beam: [R, F, 1536] per layer, loop invariant."""
        rep = [kv.repeat_interleave(self.num_beams, 0) for kv in enc_kv_all]
        if self.static:
            for e, r in zip(self.enc, rep):
                e.copy_(r)
        else:
            self._adopt([r.contiguous() for r in rep])

    def reset(self):
        """Start a search.  (static: the previous search on these buffers ended with the blocking read-out: nothing still writes the
        pinned table.)"""
        self.ibuf.zero_()
        self.ibuf[self.layout.reset].copy_(self.ibuf0)
        self.fbuf.copy_(self.fbuf0)
        self.done_rows.zero_()

    def step(self, t: int, stream):
        """Word t (1-based), one C call: the decoder step up to the LM-head logits (20 kernels), then log-softmax + beam score + top-k +
        bookkeeping + the done flags to pinned memory (2 kernels, fed the LM head's tile maxima)."""
        p = self.ptr
        _lib.check(self.lib.hirest_caption_beam_step(
            C.byref(self.desc), self.B, self.num_beams, t - 1, p.ids, p.parents, self.ptrs[t & 1] if t > 1 else None, self.ptrs[(t + 1) & 1],
            self.enc_ptrs, self.F, p.add, p.logp, self.max_words, EOS_ID, p.scores, p.tokens, p.backptr, p.n_steps, p.done,
            self.done_ptrs[t - 1], p.ws, self.buf.ws.numel(), p.tail_ws, self.buf.tail_ws.numel(), stream), "hirest_caption_beam_step")

    def step_unfused(self, t: int, stream):
        """Word t with log-softmax, top-k and beam bookkeeping as separate kernels, then the asynchronous copy of the done flags."""
        lib, p, B, nb, Vp = self.lib, self.ptr, self.B, self.num_beams, self.Vp
        _lib.check(lib.hirest_caption_decode_step(
            C.byref(self.desc), B * nb, t - 1, p.ids, p.parents if t > 1 else None, self.ptrs[t & 1] if t > 1 else None,
            self.ptrs[(t + 1) & 1], self.enc_ptrs, self.F, p.add, p.logp, p.ws, self.buf.ws.numel(), stream), "hirest_caption_decode_step")
        _lib.check(lib.hirest_topk_f32_ws(p.logp, None, B, nb * Vp, nb, p.idx, p.val, p.tk_ws, self.buf.tk_ws.numel(), stream),
                   "hirest_topk_f32_ws")
        _lib.check(lib.hirest_beam_advance(p.val, p.idx, B, nb, Vp, t - 1, self.max_words, EOS_ID, p.scores, p.tokens, p.backptr, p.n_steps,
                                           p.done, p.ids, p.parents, p.add, stream), "hirest_beam_advance")
        self.done_host[t - 1].copy_(self.buf.done, non_blocking=True)
        self.copied[t] = torch.cuda.current_stream().record_event()

    def all_done(self, t: int) -> bool:
        """Had every sample emitted [SEP] by word t?  Fused tail: the kernel stamps each sample's flag with its step — read whatever has
        arrived, never wait.  Separate kernels: the copy of word t's flags, which the caller keeps two words behind the GPU."""
        if self.fused_tail:
            return all((v >> 1) == t and (v & 1) for v in self.done_host[t - 1].tolist())
        self.copied[t].synchronize()
        return int(self.done_host[t - 1].min()) == 1

    def readout(self, return_ids):
        """The batch's synchronisation.  On the device (hirest_beam_backtrack): one [B, max_words + 1] int32 copy (length | words of the
        best beam) instead of the whole token / parent tables and a Python walk per sample (0.3 ms of host time behind a B = 32 search,
        with the GPU idle).  caption_device_readout = False: the recorded search handed to the host-side BeamState."""
        B, nb, mw, p = self.B, self.num_beams, self.max_words, self.ptr
        if self.model.caption_device_readout:
            hyp = torch.empty((B, mw + 1), dtype=torch.int32, device=self.ibuf.device)
            _lib.check(self.lib.hirest_beam_backtrack(p.scores, p.tokens, p.backptr, p.n_steps, B, nb, mw, hyp.data_ptr(), ops.stream_ptr()),
                       "hirest_beam_backtrack")
            return self.model._caption_texts([r[1:1 + r[0]] for r in hyp.cpu().tolist()], return_ids)
        L = self.layout.ibuf
        ih = self.ibuf[self.layout.readout].cpu()          # tokens | backptr | n_steps in one copy
        tok_h, bp_h = ih[L["tokens"]].view(B, mw, nb).tolist(), ih[L["backptr"]].view(B, mw, nb).tolist()
        n_h, sc_h = ih[L["n_steps"]].tolist(), self.buf.scores.view(B, -1).cpu().tolist()
        beams = [BeamState(nb) for _ in range(B)]
        for b in range(B):
            beams[b].scores = sc_h[b]
            beams[b].backptr = [bp_h[b][j] for j in range(n_h[b])]
            beams[b].tokens = [[BOS_ID] * nb] + [tok_h[b][j] for j in range(n_h[b])]
        return self.model._caption_texts([bm.best_hypothesis() for bm in beams], return_ids)


def beam_search(model, enc_kv_all, num_beams, max_words, return_ids):
    """The eager search: one BeamSearch per call, a step per word, the flags of two words ago."""
    s = BeamSearch(model, enc_kv_all[0].shape[0], num_beams, max_words, enc_kv_all[0].shape[1], len(enc_kv_all), static=False)
    s.load_encoder(enc_kv_all)
    s.reset()
    step, st = (s.step if s.fused_tail else s.step_unfused), ops.stream_ptr()
    for t in range(1, max_words + 1):
        step(t, st)
        if t >= 3 and s.all_done(t - 2):
            break
    return s.readout(return_ids)


# The same search replayed from hipGraphs (caption_batches): a word step is ~22 launches of ~3 us of host time each, and HIP
# serialises launches across host threads, so three batches in flight were HOST-bound (532 -> 766 captions/s instead of the ~2x
# the idle CUs allow).  Here all buffers of a search are static per (shape, slot), the word steps are captured once in chunks of
# CAPTION_GRAPH_CHUNK words, and a batch costs max_words / chunk graph launches.  Same kernels, same arguments, same tokens.
def graph_context(model, B, num_beams, max_words, F, nl, slot, create=False):
    """The static BeamSearch of one (shape, slot, precision); None when there is none and `create` is false."""
    ctxs = model._w().setdefault("caption_graphs", {})      # lives and dies with the weight cache: the graphs hold its pointers
    key = (B, num_beams, max_words, F, nl, slot, model.precision)
    if key not in ctxs and create:
        ctxs[key] = BeamSearch(model, B, num_beams, max_words, F, nl, static=True)
    return ctxs.get(key)


def capture(s: BeamSearch):
    """Capture the word steps of one search shape into hipGraphs (once per context; call from ONE thread while no other thread
    issues HIP work: stream capture is process-global)."""
    if s.graphs:
        return
    for e in s.enc:
        e.zero_()
    s.reset()
    for t in range(1, min(3, s.max_words) + 1):          # eager warm-up on these buffers (one-time kernel configuration must not be captured)
        s.step(t, ops.stream_ptr())
    torch.cuda.synchronize()
    chunk = max(1, int(s.model.CAPTION_GRAPH_CHUNK))
    for lo in range(1, s.max_words + 1, chunk):
        hi = min(s.max_words, lo + chunk - 1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = ops.stream_ptr()
            for t in range(lo, hi + 1):
                s.step(t, st)
        s.graphs.append((lo, hi, g))
    torch.cuda.synchronize()


def graph_beam_search(s: BeamSearch, enc_kv_all, return_ids):
    """The search on a captured context: replay a chunk, look at the flags of two chunks ago."""
    s.load_encoder(enc_kv_all)
    s.reset()
    events = []
    for k, (lo, hi, g) in enumerate(s.graphs):
        # at most two chunks ahead of the GPU, so that a search whose samples have all emitted [SEP] stops within two chunks: the
        # flags are those of the last word of chunk k - 2, which has completed (a finished sample's rows are inert meanwhile)
        if k >= 2:
            events[k - 2].synchronize()
            if s.all_done(s.graphs[k - 2][1]):
                break
        g.replay()
        events.append(torch.cuda.current_stream().record_event())
    return s.readout(return_ids)


def decoder_hidden(model, ids: torch.Tensor, enc_kv: List[torch.Tensor]) -> torch.Tensor:
    """DecoderModel.forward on whole sequences (no KV cache, like the reference; module_decoder.py:380-406 with the causal penalty
    alone, i.e. no padded key in front of a position that matters): ids [R, t] int64, enc_kv[i] [R, F, 1536] -> the last layer's
    hidden states [R * t, 768], every position."""
    c, lib = model._w(), _lib.load()
    Dp = "clip4cap_model.decoder."
    lin = lambda a, k, **kw: model._gemm(a, c[k + ".weight"], c[k + ".bias"], **kw)
    ln = lambda a, k: model._ln(a, c[k + ".LayerNorm.weight"], c[k + ".LayerNorm.bias"], 1e-12)
    (R, t), H, Dm = ids.shape, model.heads, 768
    x = torch.empty((R * t, Dm), dtype=torch.float32, device=ids.device)
    _lib.check(lib.hirest_embed_tokens(ids.contiguous().data_ptr(), c[Dp + "embeddings.word_embeddings.weight"].data_ptr(),
                                       c[Dp + "embeddings.position_embeddings.weight"].data_ptr(), x.data_ptr(), None,
                                       R, t, Dm, c[Dp + "embeddings.word_embeddings.weight"].shape[0], ops.stream_ptr()),
               "hirest_embed_tokens")
    x = ln(x, Dp + "embeddings")
    scale = (Dm // H) ** -0.5
    for i, kv in enumerate(enc_kv):
        p = Dp + f"decoder.layer.{i}."
        qkv = model._gemm(x, c[f"dec_qkv_w.{i}"], c[f"dec_qkv_b.{i}"])
        ctx = torch.empty_like(x)
        _lib.check(lib.hirest_attention_f32_qkv(qkv.data_ptr(), 3 * Dm, qkv.data_ptr() + 4 * Dm, qkv.data_ptr() + 8 * Dm, 3 * Dm,
                                                ctx.data_ptr(), R, t, t, H, Dm // H, scale, 0.0, -10000.0, ops.stream_ptr()),
                   "self attention")
        s1 = ln(lin(ctx, p + "slf_attn.output.dense", resid=x), p + "slf_attn.output")
        q2 = lin(s1, p + "enc_attn.att.query")
        _lib.check(lib.hirest_attention_f32_qkv(q2.data_ptr(), Dm, kv.data_ptr(), kv.data_ptr() + 4 * Dm, 2 * Dm, ctx.data_ptr(),
                                                R, t, kv.shape[1], H, Dm // H, scale, -10000.0, 0.0, ops.stream_ptr()), "cross attention")
        d = ln(lin(ctx, p + "enc_attn.output.dense", resid=s1), p + "enc_attn.output")
        x = ln(lin(lin(d, p + "intermediate.dense", act=1), p + "output.dense", resid=d), p + "output")
    return x


def lm_head_transform(model, rows: torch.Tensor) -> torch.Tensor:
    """BertPredictionHeadTransform (dense, GELU, LayerNorm) in front of the LM head: [n, 768] -> [n, 768]."""
    c = model._w()
    cp = "clip4cap_model.decoder.classifier.cls.predictions.transform."
    t = model._gemm(rows, c[cp + "dense.weight"], c[cp + "dense.bias"], act=1)
    return model._ln(t, c[cp + "LayerNorm.weight"], c[cp + "LayerNorm.bias"], 1e-12)


def decoder_last_logprob(model, ids: torch.Tensor, enc_kv: List[torch.Tensor], row_add: torch.Tensor) -> torch.Tensor:
    """DecoderModel.forward on the whole prefix (no KV cache, like the reference), then log_softmax of the LAST
    position + row_add (train.py:547-566, beam.py:76).  ids [R,t] int64, enc_kv[i] [R,20,1536] -> [R, vocab]."""
    c, lib = model._w(), _lib.load()
    R, t = ids.shape
    x = decoder_hidden(model, ids, enc_kv)
    last = x.reshape(R, t, x.shape[1])[:, -1, :].contiguous()             # dec_output[:, -1, :] (train.py:562)
    hh = lm_head_transform(model, last)
    logits = model._gemm(hh, c["lm_w"], c["lm_b"])
    V = logits.shape[1]
    out = torch.empty_like(logits)
    _lib.check(lib.hirest_log_softmax_f32(logits.data_ptr(), V, row_add.data_ptr(), out.data_ptr(), V, R, V, ops.stream_ptr()),
               "hirest_log_softmax_f32")
    return out


def full_prefix_search(model, enc_kv_all, num_beams, max_words, return_ids):
    """caption_kv_cache = False: the whole prefix recomputed every word and the beam bookkeeping on the host, as in the reference."""
    dev = enc_kv_all[0].device
    beams = [BeamState(num_beams) for _ in range(enc_kv_all[0].shape[0])]
    active = list(range(len(beams)))
    for t in range(1, max_words + 1):
        sel = torch.tensor([b for b in active for _ in range(num_beams)], dtype=torch.long, device=dev)
        enc_kv = [kv.index_select(0, sel).contiguous() for kv in enc_kv_all]
        # row_add = running beam scores (beam.py:76); on the first step only beam 0 competes (beam.py:78)
        add = torch.tensor([(x if (t > 1 or k == 0) else -3.0e38) for b in active
                            for k, x in enumerate(beams[b].scores)], dtype=torch.float32, device=dev)
        seqs = [s for b in active for s in beams[b].current_state()]                            # full-prefix recompute
        logp = decoder_last_logprob(model, torch.tensor(seqs, dtype=torch.long, device=dev), enc_kv, add)   # [n*beam, V]
        n, V = len(active), logp.shape[1]
        val, idx = ops.topk(logp.reshape(n, num_beams * V), num_beams)
        val_h, idx_h = val.cpu().tolist(), idx.cpu().tolist()
        active = [b for i, b in enumerate(active) if not beams[b].advance(val_h[i], idx_h[i], V)]
        if not active:
            break
    return model._caption_texts([bm.best_hypothesis() for bm in beams], return_ids)


def search(model, enc_kv_all, num_beams, max_words, return_ids, graph_slot=None):
    """The captions of one batch from its cross-attention K / V (enc_kv_all[i] [B, F, 1536] per decoder layer)."""
    if not bool(getattr(model, "caption_kv_cache", True)):
        return full_prefix_search(model, enc_kv_all, num_beams, max_words, return_ids)
    if graph_slot is not None:             # caption_batches: replay the captured word steps of this slot's context
        B, F = enc_kv_all[0].shape[0], enc_kv_all[0].shape[1]
        s = graph_context(model, B, num_beams, max_words, F, len(enc_kv_all), graph_slot)
        if s is not None and s.graphs:     # (a batch of another size, e.g. the loader's last one, runs eagerly)
            return graph_beam_search(s, enc_kv_all, return_ids)
    return beam_search(model, enc_kv_all, num_beams, max_words, return_ids)


def merge_batches(model, group, dev):
    """Several loader batches as ONE step-captioning batch: each batch is trimmed on its own (its T and its moment mask), the
    [B_i, max_frames, D] results are concatenated and the merged batch carries an all-ones moment mask — trim_feats of exactly
    max_frames selected rows is the identity, and rows a short moment left at zero stay zero.  Every kernel downstream is
    batch-invariant, so a video's caption does not depend on what it is merged with."""
    vs, as_, ts = zip(*[model._caption_inputs(b, dev) for b in group])
    v = torch.cat(vs, 0)
    merged = {"tasks": ["step_captioning"], "vis_feats": v, "moment_mask": torch.ones(v.shape[:2], dtype=torch.long),
              "text_feat": torch.cat(ts, 0)}
    if model.use_asr:
        merged["asr_feats"] = torch.cat(as_, 0)
    return merged


def caption_batches(model, batches, num_beams=5, streams=1, return_ids=False, graphs=True, merge=True, rows_in_flight=None):
    """MomentModel.caption_batches (the contract is documented there)."""
    batches = list(batches)
    if merge and len(batches) > 1:
        dev0 = model._w()["dev"]
        cap = max(1, int(rows_in_flight or model.CAPTION_ROWS_IN_FLIGHT) // max(1, num_beams))      # videos per merged search
        groups, cur, cnt = [], [], 0
        for b in batches:
            nb = int(b["vis_feats"].shape[0])
            if cur and cnt + nb > cap:
                groups.append(cur); cur, cnt = [], 0
            cur.append(b); cnt += nb
        if cur:
            groups.append(cur)
        if any(len(g) > 1 for g in groups):
            with torch.cuda.device(dev0):
                merged = [merge_batches(model, g, dev0) if len(g) > 1 else g[0] for g in groups]
            res = caption_batches(model, merged, num_beams=num_beams, streams=streams, return_ids=return_ids, graphs=graphs, merge=False)
            out = []
            for g, r in zip(groups, res):           # hand each loader batch its own slice of the merged result
                lo = 0
                for b in g:
                    nb = int(b["vis_feats"].shape[0])
                    out.append({k: v[lo:lo + nb] for k, v in r.items()})
                    lo += nb
            return out
    n = max(1, min(int(streams), len(batches)))
    dev = model._w()["dev"]                             # weight cache built (and the kernels' per-device setup done) before the threads
    if n == 1 or len(batches) <= 1:
        return [model.test_step_captioning(b, num_beams=num_beams, return_ids=return_ids) for b in batches]
    results, errors = [None] * len(batches), []
    results[0] = model.test_step_captioning(batches[0], num_beams=num_beams, return_ids=return_ids)   # warm: one-time kernel configuration
    main = torch.cuda.current_stream(dev)
    side = [torch.cuda.Stream(device=dev) for _ in range(n)]
    slot_of = lambda w: None
    if graphs and bool(getattr(model, "caption_kv_cache", True)) and fused_tail_applies(model, num_beams, model._dec_desc().vocab_padded):
        # the word steps of this batch shape, captured once per slot (hipGraphs: a batch then costs max_words / 8 launches instead
        # of ~22 per word — three host threads issuing ~3-us launches through HIP's one launch lock were the bottleneck), from this
        # thread, before the workers start
        max_frames, max_words = model._caption_limits()
        B0 = batches[1]["vis_feats"].shape[0]
        nl = len(model.clip4cap_model.decoder.decoder.layer)
        with torch.cuda.device(dev):
            for w in range(n):
                capture(graph_context(model, B0, num_beams, max_words, max_frames, nl, w, create=True))
        slot_of = lambda w: w

    def work(w):
        try:
            torch.cuda.set_device(dev)
            side[w].wait_stream(main)
            with torch.cuda.stream(side[w]):
                for i in range(1 + w, len(batches), n):
                    results[i] = model.test_step_captioning(batches[i], num_beams=num_beams, return_ids=return_ids, graph_slot=slot_of(w))
        except BaseException as e:      # surfaced after the join
            errors.append(e)
    threads = [threading.Thread(target=work, args=(w,), daemon=True) for w in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for st in side:
        main.wait_stream(st)
    if errors:
        raise errors[0]
    return results
