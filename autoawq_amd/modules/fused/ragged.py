"""Batches of prompts of different lengths: the host side of GraphedDecoder's `attention_mask` (modules/fused/decode.py).

A mask is [B, S] of 0 / 1 in the transformers convention.  Each row's ones must form ONE contiguous run (left padding,
right padding, or none).  Row b's L_b real tokens are packed to columns 0 .. L_b - 1 of a [B, max L_b] batch, so that they
get cache rows and rotary positions 0 .. L_b - 1 (transformers' `position_ids = cumsum(mask) - 1`); the pad columns behind
them repeat the row's last real token.  Causal attention means no real position ever sees a pad column, and the cache rows
the pad columns write lie at or past L_b, where the first decode step of the row overwrites or ignores them."""
import torch


def mask_runs(attention_mask, shape, max_len=None):
    """attention_mask [B, S] (0 / 1, any integer or bool dtype) -> (starts, lengths): two lists of B ints, the first column
    and the length of each row's run of ones.  Raises ValueError for a mask of the wrong shape, values other than 0 / 1,
    an all-zero row, ones that are not one contiguous run, or (with max_len) a row longer than max_len."""
    m = torch.as_tensor(attention_mask)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"attention_mask has shape {tuple(m.shape)}, input_ids {tuple(shape)}")
    m = m.detach().to("cpu")
    if m.dtype.is_floating_point or m.dtype.is_complex:
        raise ValueError("attention_mask must hold integers (0 / 1) or booleans")
    m = m.to(torch.int64)
    if bool(((m != 0) & (m != 1)).any()):
        raise ValueError("attention_mask must hold only 0 and 1")
    lengths = m.sum(1)
    # first column of the run; the run is contiguous iff the ones end exactly `length` columns later
    first = m.argmax(1)
    starts, lens = [], []
    for b in range(m.shape[0]):
        n, s = int(lengths[b]), int(first[b])
        if n == 0:
            raise ValueError(f"attention_mask row {b} has no ones: every row needs at least one token")
        if int(m[b, s:s + n].sum()) != n:
            raise ValueError(f"attention_mask row {b}: the ones must form one contiguous run (left or right padding)")
        if max_len is not None and n > max_len:
            raise ValueError(f"attention_mask row {b} has {n} tokens, more than the cache window of {max_len}")
        starts.append(s)
        lens.append(n)
    return starts, lens


def _columns(starts, lengths, width, device):
    """[B, width] source column of each packed column: start_b + min(i, L_b - 1)"""
    i = torch.arange(width, device=device).view(1, -1)
    s = torch.tensor(starts, dtype=torch.int64, device=device).view(-1, 1)
    n = torch.tensor(lengths, dtype=torch.int64, device=device).view(-1, 1)
    return s + torch.minimum(i, n - 1)


def pack_ids(input_ids, starts, lengths):
    """input_ids [B, S] -> [B, max L_b]: row b's real tokens at columns 0 .. L_b - 1, then its last real token repeated"""
    width = max(lengths)
    return input_ids.gather(1, _columns(starts, lengths, width, input_ids.device))


def unpack_rows(packed, starts, lengths, width):
    """packed [B, max L_b, ...] (logits of the packed batch) -> [B, width, ...] in the caller's layout: column start_b + i of
    row b holds packed[b, i] for i < L_b.  Pad columns hold some packed column of the same row (unspecified)."""
    B, P = packed.shape[0], packed.shape[1]
    j = torch.arange(width, device=packed.device).view(1, -1)
    s = torch.tensor(starts, dtype=torch.int64, device=packed.device).view(-1, 1)
    idx = (j - s).clamp(0, P - 1).expand(B, width)
    idx = idx.reshape((B, width) + (1,) * (packed.dim() - 2)).expand((B, width) + tuple(packed.shape[2:]))
    return packed.gather(1, idx)
