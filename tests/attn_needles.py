"""Deterministic needle inputs for the attention tests (tests/attn_bound.py has the reference and the bound).

Keys are random +-1 vectors; query head h of sequence b is c * (the key of its target row), so its score with the target is
c * 128 * scale (c = 2: ~22.6) while every other row scores c * N(0, 128) * scale (~N(0, 2^2)): the target carries nearly all of
the softmax weight, and a kernel that loses the row, or counts it twice, is off by O(|v|) in that head's output."""
import torch

D = 128


def pm1(gen, shape):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).to(torch.float16)


def decode_needles(B, Hkv, G, Tmax, targets, c=2.0, seed=0):
    """targets [B, Hq] row indices -> q [B, Hq, D], k / v caches [B, Tmax, Hkv, D] (fp16, CPU)"""
    gen = torch.Generator().manual_seed(seed)
    k = pm1(gen, (B, Tmax, Hkv, D))
    v = torch.randn((B, Tmax, Hkv, D), generator=gen).half()
    targets = torch.as_tensor(targets).reshape(B, Hkv * G)
    q = torch.empty((B, Hkv * G, D), dtype=torch.float16)
    for b in range(B):
        for h in range(Hkv * G):
            q[b, h] = (c * k[b, int(targets[b, h]), h // G].float()).half()
    return q, k, v


def deal(rows, B, Hq, start=0):
    """assign the target rows to the B * Hq slots, cycling from `start` -> ([B, Hq] targets, next start)"""
    rows = list(rows)
    t = torch.empty((B, Hq), dtype=torch.int64)
    i = start
    for b in range(B):
        for h in range(Hq):
            t[b, h] = rows[i % len(rows)]
            i += 1
    return t, i


def decode_targets(T, splits, extra=()):
    """rows 0, 15, 16, 63, 64 (the early-prefetch set), every split boundary s*chunk - 1 / s*chunk, T - 1, and `extra`, below T"""
    chunk = ((T + splits - 1) // splits + 15) & ~15
    rows = {0, 15, 16, 63, 64, T - 1}
    for s in range(1, splits):
        rows |= {s * chunk - 1, s * chunk}
    rows |= set(extra)
    return sorted(r for r in rows if 0 <= r < T)


def prefill_needles(B, S, Hq, Hkv, start, Tmax, c=2.0, seed=0, anti=True):
    """q [B, S, Hq, D], caches [B, Tmax, Hkv, D] and the target [B, S, Hq] of every query row.
    Query s targets its diagonal start + s, except rows s = 1 mod 4, which target (in turn, when visible) the KV-tile boundaries
    63 / 64 / 127 / 128, the chunk start start - 1 / start and row 0.  Anti-needles (anti=True): for s = 3 mod 4 the key of row
    start + s + 1 is twice the key of start + s, so it outscores query s's own target -- legitimate for query s + 1 (whose
    target it is), invisible to query s.  Rows 31 / 63 / 127 (wave and block boundaries) are = 3 mod 4."""
    gen = torch.Generator().manual_seed(seed)
    G = Hq // Hkv
    k = pm1(gen, (B, Tmax, Hkv, D))
    v = torch.randn((B, Tmax, Hkv, D), generator=gen).half()
    if anti:
        for s in range(3, S - 1, 4):
            k[:, start + s + 1] = k[:, start + s] * 2
    special = [63, 64, 127, 128, start - 1, start, 0]
    tgt = torch.empty((B, S, Hq), dtype=torch.int64)
    q = torch.empty((B, S, Hq, D), dtype=torch.float16)
    i = 0
    for s in range(S):
        for h in range(Hq):
            t = start + s
            if s % 4 == 1:
                # (a row whose doubled successor -- an anti-needle -- is visible too would be outscored by it)
                shadowed = lambda r: anti and start <= r < start + s and (r - start) % 4 == 3  # noqa: E731
                cand = [r for r in special if 0 <= r <= start + s and not shadowed(r)]
                t = cand[i % len(cand)]
                i += 1
            tgt[:, s, h] = t
            q[:, s, h] = (c * k[:, t, h // G].float()).half()
    return q, k, v, tgt
