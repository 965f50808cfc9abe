"""Adversarial logit rows for the sampler's kept set (csrc/sample.hip), and the witnesses that make a wrong set visible.

On Gaussian logits a kept set that is off by one token changes a draw only when that one token wins the Gumbel race (a share of
1e-4 at V = 32000).  Here the rows are built in KEY space -- the monotone 16-bit key of an fp16 logit that the kernel's two radix
rounds work on -- with at most a few dozen candidate tokens or tie groups at chosen keys and indices, and everything else filler
(-30, or -inf).  The kept set is small, every candidate has a sizeable share, and the token just inside the threshold and the one
just outside it each win a good part of a schedule of draws.

A draw schedule is `rows` identical copies of the row in ONE launch for every t of `ts`: the row index is part of the Philox
counter, so every row is an independent draw.  From the restatement alone (sampling_ref.kept_set and the scores v / T + g):
  boundary value        the smallest kept value
  first excluded value  the largest finite value that is not kept
  margin                2 TOL max(1, |best|), TOL = 1e-4: the rule of tests/test_gpu_sampling.py (fp32 scores against fp64 ones)
  decisive draw         the best kept score leads the second best kept score by more than the margin, so the token is determined
  in-witness            a decisive draw won by a token of the boundary value: a kernel that dropped that value emits something else
  out-witness           a decisive draw in which a token of the first excluded value outscores the best kept token by more than the
                        margin: a kernel that kept that value emits it, and it is not in the kept set
check_draws holds every draw to the per-draw rule (kept, score within TOL of the best, equal on a decisive draw), the token to
the restatement's on every witness, and the keys of the emitted tokens to the keys of the kept set, value group by value group.
tests/test_sampling_cases_cpu.py proves without a GPU that each case has >= 8 witnesses of either kind, that every kept value
group wins a decisive draw, and that check_draws refuses a sampler whose threshold is one value too low or too high.
(Out-witnesses need a first excluded value with a share: the bottom cases with top-k off have no excluded value, and
p_cold_zero_masses has one that cannot win -- Case.no_out says why, and the CPU test asserts that reason instead.)

Top-p margin.  The kernel's masses are exp((l - max) / T) in fp32 with |argument| <= 31 (about 4e-6 relative: the rounding of the
argument, 31 * 2^-24 * 2, and expf's), summed in 2^-43 fixed point (V * 2^-44 <= 4e-10 of Z >= 1), against top_p held as fp32
(6e-8): about 1e-5 relative in all.  Every top-p case therefore keeps the restatement's cumulative mass at least 1e-3 * Z away
from top_p * Z on both sides of the boundary -- cum(boundary value) >= (top_p + 1e-3) Z and cum(value above it) <=
(top_p - 1e-3) Z -- 100 times the kernel's error, so its boundary is the restatement's.  (top_p = 0.5 over equal masses is not
such a value.)"""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import penalty_ref as pref
import sampling_ref as ref

TOL = 1e-4          # the score tolerance of tests/test_gpu_sampling.py
P_MARGIN = 1e-3     # top-p: the distance of the cumulative mass from top_p * Z, in units of Z (derivation above)
MIN_WITNESSES = 8
ROWS = 256
SEED = 20240607
CHUNK = 2048        # elements of a row per block (kChunk)
NEG_ZERO = 0x7FFF   # the key -0 would have without the fold: bits_of_key gives 0x8000 (-0), whose key is 0x8000
V_A, V_B, V_C = 4100, 6200, 6151   # 3, 4 and 4 chunks; 6151 is odd (rows of a contiguous batch are 2-byte aligned) and its last chunk holds 7


# ---- key space ----------------------------------------------------------------------------------------------------------
def key16(bits):
    """fp16 bits -> the kernel's monotone key: larger key = larger value, -0 folded into +0; -65504 is 0x0400, -inf 0x03FF"""
    b = np.asarray(bits).astype(np.uint32) & 0xFFFF
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000).astype(np.uint32)


def bits_of_key(key):
    """the inverse (key 0x7FFF, which no value has, gives -0)"""
    k = np.asarray(key).astype(np.uint32) & 0xFFFF
    return np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint16)


def value_of_key(key):
    return bits_of_key(key).view(np.float16)


def keys_of(logits):
    return key16(np.asarray(logits, dtype=np.float16).view(np.uint16))


# ---- cases --------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class Case:
    name: str
    V: int
    raw: np.ndarray            # fp16 [V]: what the kernel is given
    logits: np.ndarray         # fp16 [V]: what the three passes read (raw, or penalty_ref.process(raw))
    temperature: float
    top_k: int
    top_p: float
    kept: np.ndarray           # the DESIGNED kept set: sorted indices, from the case's own statement, not from kept_set
    tie_free: bool             # no two candidates share a value (transformers' warpers keep the same set)
    strided: bool = False      # launched through a view whose rows are not 16-byte aligned
    ts: tuple = (1,)
    rows: int = ROWS
    seed: int = SEED
    seen: np.ndarray = None    # processors: indices in the history
    penalty: float = 1.0
    min_new: int = 0
    eos: tuple = ()
    no_out: str = ""           # why this case cannot have out-witnesses (else "")
    note: str = ""
    groups: list = field(default_factory=list)   # (processed key, indices) of the candidates

    @property
    def params(self):
        return {"temperature": self.temperature, "top_k": self.top_k, "top_p": self.top_p}


def _pool(V, rot, seed):
    """candidate indices in the order they are dealt: both ends of the row and both sides of every chunk edge first"""
    special = [0, CHUNK - 1, CHUNK, V - 1, 2 * CHUNK, 2 * CHUNK - 1] + ([3 * CHUNK, 3 * CHUNK - 1] if V > 3 * CHUNK + 1 else [])
    special = special[rot % 4:] + special[:rot % 4]
    rest = np.random.default_rng(seed).permutation(V)
    taken = set(special)
    return special + [int(i) for i in rest if int(i) not in taken]


def _build(name, V, groups, kept, *, temperature=1.0, top_k=0, top_p=1.0, filler=-30.0, strided=False, ts=(1,), seen=(),
           seen_filler=False, penalty=1.0, min_new=0, eos_group=None, no_out="", note="", rot=0):
    """groups: (key, count) of every candidate value, in any order; kept: the ordinals of the groups that are kept, by design.
    seen / eos_group: ordinals of the groups whose tokens are in the history / are EOS ids (the processors)."""
    proc = penalty != 1.0 or min_new > 0
    raw_keys = [k for k, _ in groups]
    # the processed key of every group decides who sits at the boundary; one token of the row is enough to ask penalty_ref
    probe = value_of_key(np.array(raw_keys))
    if proc:
        done = pref.process(probe, np.isin(np.arange(len(groups)), list(seen)), t=ts[0], repetition_penalty=penalty,
                            min_new_tokens=min_new, eos_ids=[eos_group] if eos_group is not None else ())
    else:
        done = probe
    pkeys = keys_of(done)
    kept = list(kept)
    out = [g for g in range(len(groups)) if g not in kept and np.isfinite(done[g])]
    b = min(kept, key=lambda g: pkeys[g])
    first = [b] + ([max(out, key=lambda g: pkeys[g])] if out else [])
    order = first + [g for g in np.argsort(-pkeys.astype(np.int64), kind="stable") if g not in first]
    pool = _pool(V, rot, len(name) + V)
    assert sum(c for _, c in groups) >= (8 if V > 3 * CHUNK + 1 else 6), name   # every special index gets a candidate
    idx = {g: [] for g in order}
    nchunks = (V + CHUNK - 1) // CHUNK
    big = [g for g in order if groups[g][1] >= 100]          # a tie group gets a token in every chunk, however short the last one
    spread = {g: [min(V, (c + 1) * CHUNK) - 2 - n for c in range(nchunks)] for n, g in enumerate(big)}
    reserved = {i for v in spread.values() for i in v}
    it = iter(i for i in pool if i not in reserved)
    for g in order:                      # one token of every group first: the boundary and the first excluded value get the specials
        idx[g].append(next(it))
    for g in order:
        idx[g] += spread.get(g, []) + [next(it) for _ in range(groups[g][1] - 1 - len(spread.get(g, [])))]
    raw = np.full(V, filler, dtype=np.float16)
    for g, (k, _) in enumerate(groups):
        raw[idx[g]] = value_of_key(k)
    seen_idx = np.array(sorted(i for g in seen for i in idx[g]), dtype=np.int64)
    if seen_filler:
        cand = {i for g in idx for i in idx[g]}
        seen_idx = np.array(sorted(set(seen_idx.tolist()) | {i for i in range(5, V, 97) if i not in cand}), dtype=np.int64)
    eos = tuple(idx[eos_group]) if eos_group is not None else ()
    logits = raw
    if proc:
        mask = np.zeros(V, dtype=bool)
        mask[seen_idx] = True
        logits = pref.process(raw, mask, t=ts[0], repetition_penalty=penalty, min_new_tokens=min_new, eos_ids=eos)
        for t in ts:
            assert (t <= min_new) == (ts[0] <= min_new), name
    used = sorted(i for g in idx for i in idx[g])
    assert {0, CHUNK - 1, CHUNK, V - 1} <= set(used) and {i // CHUNK for i in used} == set(range((V + CHUNK - 1) // CHUNK)), name
    for g, (_, c) in enumerate(groups):
        if c >= 100:                     # a tie group lies in every chunk
            assert {i // CHUNK for i in idx[g]} == set(range((V + CHUNK - 1) // CHUNK)), name
    merged = {}
    for g in range(len(groups)):
        if np.isfinite(done[g]):
            merged.setdefault(int(pkeys[g]), []).extend(idx[g])
    return Case(name=name, V=V, raw=raw, logits=logits, temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                kept=np.array(sorted(i for g in kept for i in idx[g]), dtype=np.int64),
                tie_free=all(len(v) == 1 for v in merged.values()), strided=strided, ts=tuple(ts),
                seen=seen_idx if proc else None, penalty=float(penalty), min_new=int(min_new), eos=eos, no_out=no_out, note=note,
                groups=sorted(((k, np.array(sorted(v))) for k, v in merged.items()), reverse=True))


def _run(top, n):
    """n single tokens at the consecutive keys top, top - 1, ..."""
    return [(top - j, 1) for j in range(n)]


def _make_cases():
    cases = []

    def add(name, V, groups, kept, **kw):
        cases.append(_build(name, V, groups, kept, rot=len(cases), strided=V == V_C, **kw))

    # -- top-k, the threshold inside its bin.  EDGE: 24 consecutive keys 0xC10B .. 0xC0F4 (2.52 .. 2.48) across the 0xC1 / 0xC0 edge
    edge = _run(0xC10B, 24)
    add("k_on_edge_lo00", V_A, edge, range(12), top_k=12, note="top-k threshold 0xC100: low byte 0x00, the first key of bin 0xC1")
    add("k_below_edge_loFF", V_B, edge, range(13), top_k=13, note="top-k threshold 0xC0FF: low byte 0xFF, the last key of bin 0xC0")
    add("k_above_edge_lo01", V_C, edge, range(11), top_k=11, note="top-k threshold 0xC101: the edge is one key below the cut")
    spread = [(k, 1) for k in (0xC310, 0xC2F0, 0xC280, 0xC210, 0xC1C0, 0xC180, 0xC17F, 0xC140, 0xC090, 0xC010, 0xBFC0, 0xBF00)]
    add("k_mid_bin", V_A, spread, range(6), top_k=6, note="top-k threshold 0xC180 mid-bin, candidates over six bins; 0xC17F is out")
    add("k_in_bin_of_max", V_B, _run(0xC12B, 12), range(5), top_k=5,
        note="every candidate in high byte 0xC1: the top-k bin is the bin of the maximum")

    # -- the sign crossing: +subnormals 0x8003 .. 0x8001, the zero group (+0 +0 -0 -0: one key, 0x8000), -subnormals 0x7FFE .. 0x7FFC
    zero = _run(0x8003, 3) + [(0x8000, 2), (NEG_ZERO, 2)] + _run(0x7FFE, 3)
    add("zero_k_cuts_group", V_C, zero, range(5), top_k=5, note="k = 5 cuts the zero group: +0 and -0 are one value, all four kept")
    add("zero_k_above", V_A, zero, range(3), top_k=3, note="threshold 0x8001: the zero group is the first excluded value")
    add("zero_k_exact", V_B, zero, range(5), top_k=7, note="k = 7 ends on the zero group: threshold 0x8000, the first key of bin 0x80")
    add("zero_k_below", V_C, zero, range(6), top_k=8, note="threshold 0x7FFE in bin 0x7F: the unused key 0x7FFF lies between")

    # -- the bottom of the range: an all-negative row in and just above bin 4 (kFiniteLo = 0x0400 = -65504), -inf filler.  A key
    # step is 32 there, so T = 8192 gives the eight candidates comparable shares.
    bottom = [(k, 1) for k in (0x0500, 0x04FF, 0x0480, 0x0410, 0x0408, 0x0402, 0x0401, 0x0400)]
    lo = dict(temperature=8192.0, filler=-np.inf)
    add("bottom_k_is_count", V_A, bottom, range(8), top_k=8, note="k = number of finite tokens: threshold 0x0400 itself, all kept", **lo)
    add("bottom_k_count_plus_1", V_B, bottom, range(8), top_k=9, note="k one past the finite tokens: top-k off", **lo)
    add("bottom_k_count_minus_1", V_C, bottom, range(7), top_k=7, note="threshold 0x0401: -65504 is the first excluded value", **lo)
    add("bottom_k_is_V", V_A, bottom, range(8), top_k=V_A, note="k = V over 8 finite tokens: top-k off", **lo)

    # -- a tie group across the blocks: five tokens near 5.0, 300 tokens of 1.0 in every chunk, 150 tokens one key below
    ties = _run(0xC504, 5) + [(0xBC00, 300), (0xBBFF, 150)]
    add("tie_group_top_k", V_B, ties, range(6), top_k=155, note="k = 155 cuts the group of 300 (ranks 6 .. 305): kept whole")
    add("tie_group_top_p", V_C, ties, range(6), top_p=0.6,
        note="cumulative mass 0.38 above the group, 0.79 with it: top_p = 0.6 ends inside the group, kept whole")

    # -- top-p
    add("p_top_bin", V_A, edge, range(5), temperature=0.25, top_p=0.22, note="top-p threshold 0xC107 in the bin of the maximum; T = 0.25")
    three = _run(0xC207, 16) + _run(0xC0FF, 8)
    add("p_between_bins", V_B, three, range(12), temperature=2.0, top_k=20, top_p=0.6,
        note="top bin 0xC2, top-p threshold 0xC1FC in bin 0xC1, top-k threshold 0xC0FC in bin 0xC0; T = 2")
    add("p_in_k_bin_above", V_C, edge, range(15), top_k=20, top_p=0.74,
        note="both thresholds in bin 0xC0: top-p 0xC0FD above top-k 0xC0F8")
    add("p_equals_k", V_A, edge, range(14), top_k=14, top_p=0.96, note="top-p needs all 14 that top-k keeps: both thresholds 0xC0FE")
    add("p_lo00", V_B, edge, range(12), top_p=0.48, note="top-p threshold 0xC100, low byte 0x00, top-k off")
    add("p_loFF", V_C, edge, range(13), top_p=0.52, note="top-p threshold 0xC0FF, low byte 0xFF, top-k off")
    # T = 0.05: a key step near 2.5 is 2^-9, 0.039 in units of T.  The top four and three tokens of 0xC100 carry all the mass; the
    # rest sit 46 .. 600 units below the maximum, where the kernel's fixed-point mass is 0 (< -31) and the fp64 mass is below
    # 1e-19 of Z.  With top_p = 0.999 the margin condition asks cum(boundary) >= Z (1 - 8.7e-19), i.e. exactly such a tail.
    cold = [(0xC140, 1), (0xC138, 1), (0xC130, 1), (0xC120, 1), (0xC100, 3)] + [(k, 1) for k in (0xB533, 0xB400, 0xB000, 0xA800, 0x8000, 0x4400)]
    add("p_cold_zero_masses", V_A, cold, range(5), temperature=0.05, top_p=0.999, filler=-30.0,
        no_out="the first excluded value lies 46 units of T below the maximum: its share is e^-46",
        note="T = 0.05, top_p = 0.999: every token below 0xC100 has fixed-point mass 0 and is excluded by top-p")

    # -- all three
    add("k_p_T_together", V_B, edge, range(13), temperature=0.7, top_k=20, top_p=0.63,
        note="top_k = 20 (threshold 0xC0F8), top_p = 0.63 (threshold 0xC0FF), T = 0.7")
    return cases


def _make_proc_cases():
    """the processors (penalty_ref.process is the reference of the row the passes read)"""
    cases = []
    # repetition_penalty 1.3 moves a seen logit DOWN (positive: division, negative: multiplication).  By raw value, top_k = 6:
    #   0xC010  0xC008  0xC000*  0xBF90  0xBF50*  0xBF10 | 0xBE90  0xBE10  0xBDF0 ... -1.0*          (* = in the history)
    # 0xBF50 (1.828) becomes 1.406 = 0xBDA0: out of the kept set, across the 0xBF / 0xBE and 0xBE / 0xBD edges; 0xBE90 takes its
    # place.  0xC000 (2.0) becomes 1.538 = 0xBE27 and is the new boundary value, just above the first excluded 0xBE10.
    down = [(0xC010, 1), (0xC008, 1), (0xC000, 1), (0xBF90, 1), (0xBF50, 1), (0xBF10, 1), (0xBE90, 1), (0xBE10, 1), (0xBDF0, 1),
            (0x43FF, 1)]
    cases.append(_build("penalty_moves_down", V_B, down, [0, 1, 2, 3, 5, 6], top_k=6, penalty=1.3, seen=[2, 4, 9], seen_filler=True,
                        note="repetition_penalty 1.3: the seen 0xBF50 leaves the kept set by division, the seen 2.0 becomes the boundary"))
    # repetition_penalty 0.8 moves a seen logit UP; the row is negative, so by multiplication.  By raw value, top_k = 5:
    #   0x4A00  0x49C0  0x4980  0x4940  0x4900 | 0x48C0  0x4880  0x47D6*  0x4600*
    # 0x47D6 (-0.52) becomes -0.416 in bin 0x49, between 0x4980 and 0x4940: into the kept set across the 0x47 / 0x48 and
    # 0x48 / 0x49 edges, and 0x4900 becomes the first excluded value.  0x4600 (-0.75 -> -0.6) stays out.
    up = [(0x4A00, 1), (0x49C0, 1), (0x4980, 1), (0x4940, 1), (0x4900, 1), (0x48C0, 1), (0x4880, 1), (0x47D6, 1), (0x4600, 1)]
    cases.append(_build("penalty_moves_up", V_C, up, [0, 1, 2, 3, 7], top_k=5, penalty=0.8, seen=[7, 8], seen_filler=True,
                        strided=True, note="repetition_penalty 0.8: the seen negative 0x47D6 enters the kept set by multiplication"))
    # min_new_tokens: the EOS id holds 40.0, the maximum by far.  Unprocessed, max = 40 makes every other mass exp(-37.5) = 0 in
    # fixed point; processed, max, Z and the top-p boundary come from the 24 edge candidates.
    eosrow = [(0xD100, 1)] + _run(0xC10B, 24)
    cases.append(_build("min_new_hides_max", V_A, eosrow, range(1, 13), top_p=0.48, min_new=1, eos_group=0,
                        note="min_new_tokens suppresses the EOS id that is the row maximum: max, Z and the top-p boundary are the processed row's"))
    return cases


CASES = _make_cases()
PROC_CASES = _make_proc_cases()
BY_NAME = {c.name: c for c in CASES + PROC_CASES}
assert len(BY_NAME) == len(CASES) + len(PROC_CASES)


def cases_of(V):
    return [c for c in CASES if c.V == V]


# ---- the schedule and its witnesses -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def schedule_gumbel(seed, t, rows, V):
    """g[r, i] of a launch of `rows` rows at token index t: sampling_ref.gumbel(seed, t, r, V) for every r at once.  Shared by all
    cases of one V; read-only."""
    blocks = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    r = np.arange(rows, dtype=np.uint64)[:, None]
    w = ref.philox4x64_10((np.uint64(t), r, blocks, np.uint64(0)), (np.uint64(seed), np.uint64(0)))
    u = ref.uniform_of_word(np.stack(w, axis=2).reshape(rows, -1)[:, :V]).astype(np.float64)
    g = -np.log(-np.log(u))
    g.setflags(write=False)
    return g


@dataclass
class Draws:
    keep: np.ndarray        # bool [V], sampling_ref.kept_set
    boundary: float         # the smallest kept value
    excluded: object        # the largest finite value not kept, or None
    want: np.ndarray        # [len(ts), rows] the restatement's tokens
    best: np.ndarray        # their scores
    decisive: np.ndarray    # bool: best leads the second best kept score by more than the margin
    in_w: np.ndarray        # bool
    out_w: np.ndarray       # bool


def _margin(best):
    return 2 * TOL * np.maximum(1.0, np.abs(best))


def tokens_of(case, keep):
    """the tokens of a sampler whose kept set is `keep` -> (tokens, scores, second best scores), each [len(ts), rows]"""
    x = case.logits.astype(np.float64)
    idx = np.flatnonzero(keep)
    tok, best, second = [], [], []
    for t in case.ts:
        s = x[idx] / case.temperature + schedule_gumbel(case.seed, t, case.rows, case.V)[:, idx]
        j = np.argmax(s, axis=1)                         # ties to the lowest index (idx ascends)
        tok.append(idx[j])
        best.append(s[np.arange(case.rows), j])
        second.append(np.partition(s, -2, axis=1)[:, -2] if len(idx) > 1 else np.full(case.rows, -np.inf))
    return np.array(tok), np.array(best), np.array(second)


_draws = {}


def draws(case):
    if case.name in _draws:
        return _draws[case.name]
    x = case.logits.astype(np.float64)
    keep = ref.kept_set(x, **case.params)
    boundary = x[keep].min()
    out = ~keep & np.isfinite(x)
    excluded = x[out].max() if out.any() else None
    want, best, second = tokens_of(case, keep)
    decisive = best - second > _margin(best)
    in_w = decisive & (x[want] == boundary)
    out_w = np.zeros_like(decisive)
    if excluded is not None:
        ex = np.flatnonzero(out & (x == excluded))
        for n, t in enumerate(case.ts):
            e = (x[ex] / case.temperature + schedule_gumbel(case.seed, t, case.rows, case.V)[:, ex]).max(axis=1)
            out_w[n] = decisive[n] & (e - best[n] > _margin(best[n]))
    _draws[case.name] = Draws(keep, boundary, excluded, want, best, decisive, in_w, out_w)
    return _draws[case.name]


def top_p_sides(case):
    """(cumulative mass at the boundary value, at the value above it, Z) of the restatement, over the top-k-kept set"""
    x = case.logits.astype(np.float64) / case.temperature
    kk = ref.kept_set(case.logits.astype(np.float64), case.temperature, case.top_k, 1.0)
    m = np.where(kk, np.exp(x - x[kk].max()), 0.0)
    b = draws(case).boundary / case.temperature
    return math.fsum(m[x >= b]), math.fsum(m[x > b]), math.fsum(m)   # (correctly rounded sums: independent of the order)


def top_p_margin_holds(case):
    """cum(boundary) - top_p Z >= 1e-3 Z and top_p Z - cum(above) >= 1e-3 Z, evaluated exactly on the fp64 sums"""
    at, above, z = (Fraction(v) for v in top_p_sides(case))
    p, m = Fraction(case.top_p), Fraction(P_MARGIN)
    return at - p * z >= m * z and p * z - above >= m * z


def decisive_wins(case):
    """key of a kept value group -> decisive draws it wins"""
    d = draws(case)
    k = keys_of(case.logits)
    won = k[d.want[d.decisive]]
    return {int(key): int((won == key).sum()) for key in np.unique(k[d.keep])}


def check_draw(case, tok, *, seed, t, row, do_sample=True):
    """the per-draw rule for one row of a launch with parameters of its own (tests/test_gpu_sampling.py: _check_sampled)"""
    want, keep, s = ref.choose(case.logits, do_sample=do_sample, seed=seed, t=t, row=row, **case.params)
    if not do_sample:
        assert tok == want, (case.name, row, tok, want)
        return 0.0
    assert 0 <= tok < case.V and keep[tok], (case.name, row, tok, want)
    best = s[want]
    assert abs(s[tok] - best) <= TOL * max(1.0, abs(best)), (case.name, row, tok, want, s[tok], best)
    runner_up = np.sort(s[np.isfinite(s)])[-2] if np.isfinite(s).sum() > 1 else -np.inf
    if best - runner_up > 2 * TOL * max(1.0, abs(best)):
        assert tok == want, (case.name, row, tok, want)
    return abs(s[tok] - best) / (TOL * max(1.0, abs(best)))


def check_draws(case, tokens):
    """tokens [len(ts), rows] of the case's schedule.  Raises AssertionError; returns what SAMPLING_KEPT_RECORD records."""
    d = draws(case)
    tokens = np.asarray(tokens, dtype=np.int64).reshape(len(case.ts), case.rows)
    x = case.logits.astype(np.float64)
    inside = (tokens >= 0) & (tokens < case.V)
    assert inside.all(), (case.name, "a token outside [0, V)", tokens[~inside][:4])
    kept = d.keep[tokens]
    assert kept.all(), (case.name, "emitted a token that is not kept", np.argwhere(~kept)[:4].tolist(), tokens[~kept][:4].tolist(),
                        x[tokens[~kept][:4]].tolist())
    gap = np.empty(tokens.shape)
    for n, t in enumerate(case.ts):
        g = schedule_gumbel(case.seed, t, case.rows, case.V)
        gap[n] = d.best[n] - (x[tokens[n]] / case.temperature + g[np.arange(case.rows), tokens[n]])
    rel = np.abs(gap) / np.maximum(1.0, np.abs(d.best))
    assert (rel <= TOL).all(), (case.name, "score further than TOL from the best", float(rel.max()))
    wrong = d.decisive & (tokens != d.want)
    assert not wrong.any(), (case.name, "another token on a decisive draw", np.argwhere(wrong)[:4].tolist(), tokens[wrong][:4].tolist(),
                             d.want[wrong][:4].tolist())
    # over the schedule: the witnesses (decisive draws, so this restates the line above for the draws that carry the proof) ...
    for kind, w in (("in", d.in_w), ("out", d.out_w)):
        assert (tokens[w] == d.want[w]).all(), (case.name, kind + "-witness draw lost")
    # ... and the set that was seen is the set that is kept, value group by value group
    k = keys_of(case.logits)
    seen, kept_keys = set(k[tokens.reshape(-1)].tolist()), set(k[d.keep].tolist())
    assert seen == kept_keys, (case.name, "never emitted", sorted(hex(v) for v in kept_keys - seen), "emitted outside",
                               sorted(hex(v) for v in seen - kept_keys))
    return {"in_witnesses": int(d.in_w.sum()), "out_witnesses": int(d.out_w.sum()), "worst_gap_over_tol": float(rel.max() / TOL)}
