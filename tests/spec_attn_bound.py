"""The attention error bound of tests/attn_bound.py for awq_verify_attention_rows (csrc/verify_attn.hip).

What differs from the decode class, and what does not.  The verify kernel is the decode kernel's ROWS form with (head, token) pairs
in the place of heads: per pair it runs the SAME arithmetic -- q * scale in fp32, 8 fmas and the 16-lane butterfly
(n_dot = DECODE_N_DOT = 14), one online-softmax chain per lane group over the rows t0 + o + 16 i of its split, 2 lane-group merges,
the 4-wave running sum, the combine kernel's running sum over the splits.  The rows are dealt to the splits from the SEQUENCE's
length pos_b + T for every pair (a pair that sees fewer rows walks fewer steps of the same chunk, so its depths are at most those),
hence N and n_exp are attn_bound.decode_depths(pos_b + T, splits) for every pair of sequence b: the formula is reused unchanged.
The only new number is the launch's split count: the decode rule with the token groups counted as blocks (verify_splits below,
cross-checked against awq_verify_attention_splits).  Visibility is per pair: query (b, j) sees rows t <= min(pos_b + j, Tmax - 1),
which is exactly attn_bound.reference's pos[b, r]."""
import torch

import attn_bound as ab


def group_tokens(G, T):
    """tokens per block: the smallest power of two >= T with G * TT <= 8"""
    tt = 1
    while tt < T and G * tt * 2 <= 8:
        tt *= 2
    return tt


def verify_splits(max_len, B, T, Hq, Hkv):
    tt = group_tokens(Hq // Hkv, T)
    ng = (T + tt - 1) // tt
    splits = 1 if max_len <= 256 else (max_len + 127) // 128
    splits = min(splits, max(1024 // (B * Hkv * ng), 1), 64)
    return max(splits, 1)


def verify_pos(pos_rows, T, Tmax):
    p = torch.as_tensor(pos_rows).to(torch.int64).reshape(-1, 1) + torch.arange(T).view(1, T)
    return p.clamp(0, Tmax - 1)


def verify_bound(q, k, v, pos_rows, splits, drop=None, pos=None):
    """q [B, T, Hq, D], caches [B, Tmax, Hkv, D], pos_rows [B].  Returns (want, bound), both [B, T, Hq, D] float64.
    pos [B, T]: another visibility than the kernel's (the anti-needle check asks what the output WOULD be one row further)."""
    B, T = q.shape[0], q.shape[1]
    Tmax = k.shape[1]
    lens = [int(min(int(p) + T - 1, Tmax - 1)) + 1 for p in torch.as_tensor(pos_rows).tolist()]
    depth, n_exp = zip(*(ab.decode_depths(L, splits) for L in lens))
    fn = lambda r: ab._bound(r, ab.DECODE_N_DOT, list(depth), list(n_exp), prefill=False)  # noqa: E731
    if pos is None:
        pos = verify_pos(pos_rows, T, Tmax)
    return ab._chunked(q, k, v, pos, None, 0.0, None, drop, fn)
