"""Speculative decoding restated in numpy: the acceptance rule of awq_spec_accept and the prompt-lookup drafts of awq_ngram_draft
(include/awq_hip.h), and the two generation loops built from them.  Integer code: the kernels agree with it exactly."""
import numpy as np


def accept(inp, pred, cnt, max_new_tokens, eos_ids=()):
    """inp [T] the step's input tokens, pred [T] the greedy argmax at every slot, cnt the tokens generated so far.
    Returns (new tokens, finished)."""
    T = len(inp)
    a = 0
    while a < T - 1 and int(inp[a + 1]) == int(pred[a]):
        a += 1
    new = []
    finished = False
    for j in range(a + 1):
        if len(new) >= max_new_tokens - cnt:
            break
        new.append(int(pred[j]))
        if int(pred[j]) in eos_ids:
            finished = True
            break
    return new, finished or cnt + len(new) >= max_new_tokens


def draft(h, T, ngram_max):
    """h: every token of the row (prompt, then generated), n >= 1 -> the next step's input [T]: h[-1], then T - 1 drafts"""
    h = [int(x) for x in h]
    n = len(h)
    out = [h[n - 1]] * T
    for g in range(ngram_max, 0, -1):
        if n <= g:
            continue
        for s in range(n - g - 1, -1, -1):  # the largest s first
            if h[s:s + g] == h[n - g:n]:
                for i in range(T - 1):
                    if s + g + i < n:
                        out[1 + i] = h[s + g + i]
                return out
    return out


def accept_state(state, tok, pred, params, status_bad=None):
    """awq_spec_accept on a dict of numpy arrays (hist, n_hist, cnt, ring, finished, pos_rows, len_rows), in place"""
    B, T = tok.shape
    for b in range(B):
        if state["finished"][b]:
            continue
        if status_bad is not None and status_bad[b]:
            state["finished"][b] = 1
            continue
        new, fin = accept(tok[b], pred[b], int(state["cnt"][b]), params["max_new_tokens"], params["eos"])
        c, n = int(state["cnt"][b]), int(state["n_hist"][b])
        for i, t in enumerate(new):
            if c + i < state["ring"].shape[1]:
                state["ring"][b, c + i] = t
            if n + i < state["hist"].shape[1]:
                state["hist"][b, n + i] = t
        m = len(new)
        for k in ("cnt", "n_hist", "pos_rows", "len_rows"):
            state[k][b] += m
        if fin:
            state["finished"][b] = 1


def greedy_loop(f, prompt, max_new_tokens, eos_ids=()):
    """f(prefix list) -> next token: the plain loop"""
    h = list(prompt)
    out = []
    while len(out) < max_new_tokens:
        t = f(h)
        out.append(t)
        h.append(t)
        if t in eos_ids:
            break
    return out


def spec_loop(f, prompt, max_new_tokens, T, ngram_max, eos_ids=()):
    """the speculative loop: token 1 plainly, then steps of T tokens.  Returns (tokens, tokens emitted by each step)"""
    h = list(prompt)
    first = f(h)
    h.append(first)
    out, per_step = [first], []
    finished = first in eos_ids or max_new_tokens <= 1
    while not finished:
        inp = draft(h, T, ngram_max)
        base = h[:-1]
        pred = [f(base + inp[:j + 1]) for j in range(T)]   # slot j: the model after the step's first j + 1 tokens
        new, finished = accept(inp, pred, len(out), max_new_tokens, eos_ids)
        assert len(new) >= 1
        out += new
        h += new
        per_step.append(len(new))
    return out, per_step
