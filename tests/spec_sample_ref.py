"""The slot rule of awq_sample_tokens_slots and the history OR of awq_spec_accept_ex (include/awq_hip.h) restated with the
existing restatements: a slot (b, j) of a verify step is the plain sampler (sampling_ref.choose on penalty_ref.process) for
request b at token index cnt[b] + 1 + j, with the drafts in front of the slot added to the ids seen."""
import numpy as np

import penalty_ref as pref
import sampling_ref as ref
import spec_ref


def slot_seen(history_row, tok_row, j, V):
    """bool [V]: history row b's bits OR the drafts tok[b, 1 .. j] (ids outside [0, V) ignored)"""
    seen = pref.seen_mask(history_row, V).copy()
    for d in tok_row[1:j + 1]:
        if 0 <= int(d) < V:
            seen[int(d)] = True
    return seen


def slot_logits(logits_row, history_row, tok_row, j, cnt, *, repetition_penalty=1.0, min_new_tokens=0, eos_ids=()):
    """the processed fp16 values slot j reads: t = cnt + 1 + j, seen = history OR the drafts before the slot"""
    V = len(logits_row)
    return pref.process(logits_row, slot_seen(history_row, tok_row, j, V), t=int(cnt) + 1 + j,
                        repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, eos_ids=eos_ids)


def slot_choose(logits_row, history_row, tok_row, j, cnt, b, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                repetition_penalty=1.0, min_new_tokens=0, eos_ids=()):
    """sampling_ref.choose for slot (b, j): (token or None, kept mask, scores); the Philox row is the request b"""
    v = slot_logits(logits_row, history_row, tok_row, j, cnt, repetition_penalty=repetition_penalty,
                    min_new_tokens=min_new_tokens, eos_ids=eos_ids)
    return ref.choose(v, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, t=int(cnt) + 1 + j, row=b)


def accept_state(state, tok, pred, params, status_bad=None, history=None, V=None):
    """spec_ref.accept_state, and -- awq_spec_accept_ex -- the bit of every token a row emits set in its history row (uint32 /
    int32 words [B, >= ceil(V / 32)], in place); ids outside [0, V) set nothing, finished and status-bit rows touch nothing"""
    B = tok.shape[0]
    emitted = [[] for _ in range(B)]
    for b in range(B):
        if state["finished"][b] or (status_bad is not None and status_bad[b]):
            continue
        emitted[b], _ = spec_ref.accept(tok[b], pred[b], int(state["cnt"][b]), params["max_new_tokens"], params["eos"])
    spec_ref.accept_state(state, tok, pred, params, status_bad=status_bad)
    if history is not None:
        w = history.view(np.uint32)
        for b, new in enumerate(emitted):
            for t in new:
                if 0 <= t < V:
                    w[b, t >> 5] |= np.uint32(1 << (t & 31))
    return emitted
