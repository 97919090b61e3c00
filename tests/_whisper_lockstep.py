"""The lock-step sampling loop of one window, as whisper.decode() ran it before it moved onto the per-row loop: every candidate row at
the same position, TextDecoder.prefill, then hirest_whisper_step_tail + TextDecoder.step per token.  tests/test_gpu_whisper_dec.py pins
these pieces to fp64 transformers, so this is the yardstick the per-row loop behind decode() / decode_many() is held equal to."""
import ctypes as C

import torch

from hirest_amd import _lib, ops, whisper


@torch.no_grad()
def lockstep_decode(model, window_states, options):
    """encoder states [Tk, D] of one window -> ([(tokens, sum_logprobs) of every candidate], no_speech_prob)"""
    tokenizer, dec, dev, lib = model.tokenizer, model.decoder, model.device, _lib.load()
    Vp = dec.vocab_padded
    with torch.cuda.device(dev):
        initial, sot_index = whisper._initial_tokens(tokenizer, options, dec.ctx)
        sample_begin = len(initial)
        group = (options.best_of or 1) if options.temperature > 0 else 1
        T_max = min(dec.ctx, sample_begin + (options.sample_len or dec.ctx // 2))
        steps = T_max - sample_begin
        assert steps > 0
        kc = whisper.KVCache(dec, window_states[None].to(dev, torch.float32), torch.zeros(group, dtype=torch.int32), T_max)
        params, mask = whisper.tail_params(tokenizer, options, dec.vocab, Vp, model.dims["n_audio_ctx"], 0, dev)
        padded = dec.prefill(torch.tensor([initial], dtype=torch.int32), kc)                        # [T, vocab_padded]
        state = whisper.new_row_state(group, dev)
        tokens = torch.full((group, steps), tokenizer.eot, dtype=torch.int32, device=dev)
        ids = torch.empty((group,), dtype=torch.int32, device=dev)
        stamp = torch.zeros(1, dtype=torch.int32).pin_memory()
        logits = padded[sample_begin - 1].expand(group, -1).contiguous()
        no_speech = state
        if sot_index != sample_begin - 1 and tokenizer.no_speech is not None:                       # read at the sot position, into a scratch state
            no_speech, sid = whisper.new_row_state(1, dev), torch.empty(1, dtype=torch.int32, device=dev)
            row = padded[sot_index].contiguous()
            _lib.check(lib.hirest_whisper_step_tail(row.data_ptr(), Vp, 1, Vp, 0, 0, C.byref(params), no_speech.data_ptr(), sid.data_ptr(), None,
                                                    None, None, ops.stream_ptr()), "hirest_whisper_step_tail")
        for step in range(steps):
            params.serial = step
            _lib.check(lib.hirest_whisper_step_tail(logits.data_ptr(), Vp, group, Vp, step, steps, C.byref(params), state.data_ptr(),
                                                    ids.data_ptr(), tokens.data_ptr(), None, stamp.data_ptr(), ops.stream_ptr()),
                       "hirest_whisper_step_tail")
            if (int(stamp[0]) & 1) or step == steps - 1:              # whatever step has landed by now: no wait
                break
            logits = dec.step(ids, kc)
        torch.cuda.current_stream().synchronize()
        toks, sums = tokens.cpu().tolist(), state.cpu()[:, 5].view(torch.float32).tolist()
        cands = [(row[:row.index(tokenizer.eot)] if tokenizer.eot in row else row, sums[g]) for g, row in enumerate(toks)]
        return cands, no_speech.cpu()[0, 6:7].view(torch.float32).item()
