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


def mask_runs_extend(attention_mask, shape):
    """`mask_runs` for GraphedDecoder.extend, where a row may bring no token at all: an all-zero row is (start 0, length 0).
    Everything else is refused as there (shape, values other than 0 / 1, ones that are not one contiguous run); the window
    is the caller's check -- it depends on where each row stands."""
    m = torch.as_tensor(attention_mask)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"attention_mask has shape {tuple(m.shape)}, input_ids {tuple(shape)}")
    m = m.detach().to("cpu")
    if m.dtype.is_floating_point or m.dtype.is_complex:
        raise ValueError("attention_mask must hold integers (0 / 1) or booleans")
    m = m.to(torch.int64)
    if bool(((m != 0) & (m != 1)).any()):
        raise ValueError("attention_mask must hold only 0 and 1")
    starts, lens = [], []
    for b in range(m.shape[0]):
        n = int(m[b].sum())
        s = int(m[b].argmax()) if n else 0
        if int(m[b, s:s + n].sum()) != n:
            raise ValueError(f"attention_mask row {b}: the ones must form one contiguous run (left or right padding)")
        starts.append(s)
        lens.append(n)
    return starts, lens


def generate_tail(lengths, ring, eos, n, idle=()):
    """What a `generate` call leaves behind, per row: (cache_rows, pending).  lengths[b]: the cache rows of row b when token 1
    was sampled (its prompt); ring[b][:n]: the n tokens the call sampled for it -- the row's real tokens up to and including its
    first EOS id, pads from then on; rows in `idle` started finished and emitted pads only.  Token i + 1 is sampled by the step
    that feeds token i, so ring[b][:n - 1] were fed (appended to the cache, real tokens and pads alike) and ring[b][n - 1] was not.
      cache_rows[b] = lengths[b] + the real tokens that were fed: the rows above hold pads and are dead;
      pending[b]    = the last real token if it was not fed (the row never finished, or finished on token n), else None.
    Pure host code: lists or a CPU tensor in, two lists out (a ring that holds fewer than n tokens, or n < 1: ValueError)."""
    B = len(lengths)  # (the uniform case of generate_tail_rows: every row the same EOS ids and the budget n)
    return _tail_rows("generate_tail", lengths, ring, [eos] * B, [n] * B, n, idle)[:2]


def generate_tail_rows(lengths, ring, eos_rows, max_rows, n, idle=()):
    """generate_tail for a call with per-row arguments: row b has its own EOS ids eos_rows[b] and its own budget max_rows[b], and
    the call sampled n = min(max(max_rows), where the host stopped) tokens for every row.  Returns (cache_rows, pending, real);
    real[b]: the row's real tokens -- up to and including its first EOS id, at most max_rows[b].  A row that used up a budget
    below n has fed its last token to a decode step; it is still handed back as pending with the cache row under it dead, which is
    where a call with that budget for every row leaves it (the token is then fed again by the next turn's extend)."""
    return _tail_rows("generate_tail_rows", lengths, ring, eos_rows, max_rows, n, idle)


def _tail_rows(fn, lengths, ring, eos_rows, max_rows, n, idle):
    """generate_tail_rows' body; fn: the public function named in the refusal"""
    cache_rows, pending, reals = [], [], []
    for b, L in enumerate(lengths):
        row = [int(t) for t in ring[b][:n]]
        if len(row) != n or n < 1:
            raise ValueError(f"{fn}: row {b} of the ring holds {len(row)} tokens, n = {n}")
        eos = set(int(e) for e in eos_rows[b])
        m = min(int(max_rows[b]), n)
        if b in idle:
            real, by_eos = 0, True
        else:
            real = next((i + 1 for i, t in enumerate(row[:m]) if t in eos), None)
            by_eos = real is not None
            real = real if by_eos else m
        if by_eos:
            cache_rows.append(int(L) + min(real, n - 1))
            pending.append(row[n - 1] if real == n else None)
        else:
            cache_rows.append(int(L) + real - 1)
            pending.append(row[real - 1])
        reals.append(real)
    return cache_rows, pending, reals


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
