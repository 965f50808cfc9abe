"""float64 reference, crafted router logits and checkers for the MoE routing code, for the tests: awq_moe_route_kernel /
awq_moe_sort_kernel / awq_silu_and_mul_kernel (autoawq_amd/csrc/elementwise.hip), their torch restatements ops.fused_topk /
ops.moe_align_block_size, ep.local_routing, and the dispatch of modules/fused/moe.py.

Reference.  `route_ref(logits_f32, k, renorm)`: softmax in float64 of the fp32 logits; the k experts by descending LOGIT with a
stable sort (the lowest index wins a tie -- the rule elementwise.hip:45 documents and oracle.moe_forward's stable argsort has), ids
in selection order; optional renormalisation by the sum of the k chosen weights.  NaN / Inf logits are not cases: what the kernels
and the references do with them is undefined (torch.topk, numpy's argsort and the butterfly each place a NaN where they like),
and nothing here tests it.

Decidability.  `decidable(logits)`: any two logits of a row are bit-equal or at least 2^-12 apart, and a row's spread is at most
80.  Then exp(lg - mx) is a normal fp32 number (exp(-80) = 1.8e-35; times 1 / sum >= 1 / 64 still normal), two different logits
give values that differ by a relative 2.4e-4 -- thousands of fp32 ulps, so no rounding of the subtraction or of expf reorders or
merges them -- and equal logits give equal bits.  The float64 reference alone fixes the ids: tests compare them with array_equal
and leave no row out.  Every case family below is decidable by construction and every test asserts it.

Weight bound, counted from elementwise.hip:73-106.  u = 2^-24, gamma(n) = n u / (1 - n u) (tests/matmul_bound.py), d_e = lg_e - mx,
p = the exact softmax, 1.01 for the second-order products of the first-order terms (all below 1e-4).
    * :74-78  `lg - mx` is one fp32 subtraction, (lg - mx)(1 + delta): the exponential moves by a relative |d_e| u.  The butterfly
      maximum (:75-77) is exact.  expf: the HIP math API states 1 ulp = 2 u.                       a_e = (|d_e| + 2) u
    * :79-80  the denominator adds the E values in sequence from 0.f: E - 1 roundings on positive terms, each term off by its own
      a_x:                                                                             den = sum_x p_x a_x + gamma(E - 1)
    * :81     `1.0f / sum`: 2.5 ulp where the division is not correctly rounded (the count tests/matmul_bound.py takes for
      awq_silu_mul_f32's division):                                                                             DIV = 5 u
    * :97     `bv * inv`: u.
  renorm = 0 (:105 stores `mine`):      |w~ - w| <= 1.01 w (a_e + den + DIV + u)
    * :98     wsum adds the k products in sequence from 0.f: gamma(k) on positive terms (k - 1 roundings, counted as k).
    * :105    `mine / wsum`: DIV.
  renorm = 1: every product carries the SAME factor inv (one register), which cancels in the quotient, and with it den and the
  first DIV.  With q = the exact renormalised weights of the row:
                                        |w~ - w| <= 1.01 w (a_e + u + sum_j q_j (a_j + u) + gamma(k) + DIV)
First order this is (|d_e| + sum p |d| + E + 9) u without and (|d_e| + sum q |d| + k + 11) u with renormalisation.  The float32
numpy restatement of the kernel in tests/test_moe_route_ref_cpu.py stays below a quarter of it on every family; that is a check of
the counting, not its source.

silu.  `silu_mul_ref(gate_up)` = silu(gate) up in float64 with the bound ulp16(want) / 2 (1 + 2^-10) + 1.01 gamma(16) |want|:
awq_silu_mul_f32's four fp32 operations are gamma(SILU_N) (derived in tests/matmul_bound.py and imported from there), then ONE
rounding to fp16 of a value that far from want.

Case families (`build(family, T, E, k, seed, block, e0, nl)` -> fp32 logits [T, E], or None where the shape cannot carry the
family, e.g. `empties` with k > 2):
    ties          multiples of 0.25 in [-1, 1]: many bit-equal values in a row
    all_equal     one value everywhere: expert j is the j-th choice of every token, weights 1 / E (1 / k renormalised)
    near          1 + {0, 1, 2} 2^-12
    spread        a row's maximum is 0, the others go down to -80 in steps of 0.25 (second=-60: the runner-up sits there)
    big / neg     +-30000 plus multiples of 0.5: without the maximum subtracted expf overflows / underflows
    crowded       every token puts the same two experts on top, 0.7 / 0.3 after renormalisation; the rest keep real mass
    one_mod_block every (local) expert's pair count is 1 (mod block): the padded length is P_owned + nl (block - 1), the capacity
    multiple      every (local) expert's pair count is a multiple of the block (no padding slot at all)
    empties       only experts {0, E - 1} are ever chosen
"""
import numpy as np

from matmul_bound import SILU_N, U, gamma, ulp16

DIV = 5.0 * U        # a division that is not correctly rounded: 2.5 ulp (HIP math API)
EXPF = 2.0 * U       # expf: 1 ulp
MIN_GAP = 2.0 ** -12
MAX_SPREAD = 80.0
FAMILIES = ("ties", "all_equal", "near", "spread", "big", "neg", "crowded", "one_mod_block", "multiple", "empties")
NO_TIES = ("spread_distinct", "big", "neg", "crowded")  # see build(): families (or variants) whose rows hold no two equal logits


# ------------------------------------------------------------------ reference

def route_ref(logits_f32, k, renorm):
    """(weights [T, k] float64, ids [T, k] int32 in selection order)"""
    lg = np.asarray(logits_f32)
    assert lg.dtype == np.float32 and lg.ndim == 2 and 1 <= k <= lg.shape[1]
    l64 = lg.astype(np.float64)
    p = np.exp(l64 - l64.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    ids = np.argsort(-l64, axis=-1, kind="stable")[:, :k]
    w = np.take_along_axis(p, ids, -1)
    if renorm:
        w = w / w.sum(-1, keepdims=True)
    return w, ids.astype(np.int32)


def decidable(logits):
    """any two logits of a row bit-equal or >= 2^-12 apart, the row's spread <= 80, everything finite"""
    lg = np.asarray(logits)
    if lg.dtype != np.float32 or lg.ndim != 2 or not np.isfinite(lg).all():
        return False
    if np.signbit(lg[lg == 0]).any():  # +0 and -0 compare equal with different bits: no family produces -0
        return False
    s = np.sort(lg.astype(np.float64), axis=-1)
    gap = np.diff(s, axis=-1)  # (a gap of 0 between finite values of one sign of zero: the same bits)
    return bool(((gap >= MIN_GAP) | (gap == 0)).all() and (s[:, -1] - s[:, 0] <= MAX_SPREAD).all())


def weight_bound(logits_f32, k, renorm):
    """(want [T, k] float64, ids [T, k] int32, bound [T, k] float64) -- the module docstring's count"""
    lg = np.asarray(logits_f32)
    E = lg.shape[1]
    want, ids = route_ref(lg, k, renorm)
    l64 = lg.astype(np.float64)
    d = np.abs(l64 - l64.max(-1, keepdims=True))
    p = np.exp(-d)
    p = p / p.sum(-1, keepdims=True)
    a = d * U + EXPF                                      # [T, E]: the subtraction and expf
    a_sel = np.take_along_axis(a, ids.astype(np.int64), -1)
    if not renorm:
        den = (p * a).sum(-1, keepdims=True) + gamma(E - 1)
        rel = a_sel + den + DIV + U
    else:
        rel = a_sel + U + (want * (a_sel + U)).sum(-1, keepdims=True) + gamma(k) + DIV
    return want, ids, 1.01 * rel * want


def check_route(logits_f32, k, renorm, w, ids, what=""):
    """ids equal the reference exactly (every row), weights within the derived bound; returns the largest err / bound"""
    want, wid, bnd = weight_bound(logits_f32, k, renorm)
    ids = np.asarray(ids)
    assert ids.shape == wid.shape and ids.dtype == np.int32, (what, ids.shape, ids.dtype)
    if not np.array_equal(ids, wid):
        rows = np.nonzero((ids != wid).any(-1))[0]
        t = int(rows[0])
        raise AssertionError(f"{what}: ids differ from the reference in {rows.size} of {ids.shape[0]} rows; row {t}: got {ids[t].tolist()}, "
                             f"want {wid[t].tolist()}, logits {np.asarray(logits_f32)[t].tolist()}")
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.shape == want.shape, (what, w.dtype, w.shape)
    err = np.abs(w.astype(np.float64) - want)
    bad = ~(err <= bnd)
    if bad.any():
        t, j = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} weights outside the derived bound; ({t},{j}): got {w[t, j]!r}, want "
                             f"{want[t, j]!r}, err {err[t, j]:.3g} = {err[t, j] / bnd[t, j]:.3g} x bound")
    return float((err / bnd).max())


# ------------------------------------------------------------------ alignment and sort

def _oracle():
    from oracle import awq_oracle

    awq_oracle.build()
    return awq_oracle


def check_alignment(ids, E, block, sorted_ids, expert_ids, npad, e0=0, nl=None, parked=False):
    """The block alignment of the pairs of `ids` [T, k] (global expert ids) owned by experts [e0, e0 + nl): equality with
    oracle.moe_align of the owned pairs renumbered to [0, nl), AND the invariants themselves.  The whole of sorted_ids is looked at.
    parked=True is ep.local_routing's documented form: the foreign pairs sit in one extra bucket right after npad (ascending, padded
    to the block), which the caller cuts off with npad; that bucket is checked too, and everything after it is the sentinel."""
    ids = np.asarray(ids).reshape(-1)
    nl = E - e0 if nl is None else nl
    assert 0 <= e0 and nl >= 1 and e0 + nl <= E and block >= 1
    P = ids.size
    sorted_ids, expert_ids = np.asarray(sorted_ids), np.asarray(expert_ids)
    assert sorted_ids.dtype == np.int32 and expert_ids.dtype == np.int32 and sorted_ids.ndim == 1 and expert_ids.ndim == 1
    npad = int(np.asarray(npad).reshape(-1)[0])
    owned = (ids >= e0) & (ids < e0 + nl)
    rel = np.where(owned, ids - e0, nl).astype(np.int32)   # the oracle walks experts [0, nl): bucket nl is never placed
    ws, we, wn = _oracle().moe_align(rel, nl, block)
    cap = P + nl * (block - 1)
    assert ws.size == cap
    assert npad == wn, f"num_tokens_post_padded {npad}, want {wn}"
    assert npad % block == 0 and npad <= cap
    if parked:
        assert sorted_ids.size >= cap
        foreign = np.nonzero(~owned)[0].astype(np.int32)
        tail = np.full(sorted_ids.size - npad, P, np.int32)
        tail[: foreign.size] = foreign
        assert np.array_equal(sorted_ids[npad:], tail), "the parked bucket is not the foreign pairs in order, then the sentinel"
        sorted_ids = np.concatenate([sorted_ids[:npad], np.full(cap - npad, P, np.int32)])
    assert sorted_ids.size == cap, f"sorted_token_ids holds {sorted_ids.size} slots, the capacity is {cap}"
    assert np.array_equal(sorted_ids, ws), f"sorted_token_ids differs from the oracle at slots {np.nonzero(sorted_ids != ws)[0][:8].tolist()}"
    nb = npad // block
    assert expert_ids.size >= nb
    assert np.array_equal(expert_ids[:nb], we[:nb]), f"expert_ids {expert_ids[:nb].tolist()}, want {we[:nb].tolist()} (relative to {e0})"
    # the invariants, directly
    assert (sorted_ids[npad:] == P).all(), "a slot at or past num_tokens_post_padded is not the sentinel"
    eb = expert_ids[:nb]
    assert ((eb >= 0) & (eb < nl)).all() and (np.diff(eb) >= 0).all(), "expert_ids not relative to the first expert, or decreasing"
    placed = []
    for b in range(nb):
        run = sorted_ids[b * block:(b + 1) * block]
        real = run[run != P]
        assert ((real >= 0) & (real < P)).all(), "a padding slot that is not the sentinel"
        assert (run[: real.size] == real).all(), "padding inside a block's run"
        assert real.size > 0, "a block without a pair"
        assert (ids[real] == e0 + eb[b]).all(), "a pair in a block of another expert"
        placed.append(real)
    placed = np.concatenate(placed) if placed else np.zeros(0, np.int32)
    for e in range(nl):
        run = placed[ids[placed] == e0 + e]
        assert (np.diff(run) > 0).all(), f"expert {e0 + e}: pairs not in ascending order"
        assert run.size == int((ids == e0 + e).sum()), f"expert {e0 + e}: {run.size} pairs placed"
        # only the expert's LAST block may hold padding
        blocks = np.nonzero(eb == e)[0]
        for b in blocks[:-1]:
            assert (sorted_ids[b * block:(b + 1) * block] != P).all(), f"expert {e0 + e}: padding before its last block"
    assert placed.size == int(owned.sum())


def check_sort(ids, E, order, seg):
    """awq_moe_sort_kernel's contract: seg [E + 1] = the exclusive cumulative sum of the bincount of the ids inside [0, E);
    order[: seg[E]] = the stable argsort of those pairs (pairs of other ids are not placed)"""
    ids = np.asarray(ids).reshape(-1)
    order, seg = np.asarray(order), np.asarray(seg)
    assert order.dtype == np.int32 and seg.dtype == np.int32 and seg.shape == (E + 1,) and order.shape == ids.shape
    valid = (ids >= 0) & (ids < E)
    wseg = np.zeros(E + 1, np.int64)
    wseg[1:] = np.cumsum(np.bincount(ids[valid], minlength=E))
    assert np.array_equal(seg, wseg), f"seg {seg.tolist()}, want {wseg.tolist()}"
    n = int(wseg[E])
    key = np.where(valid, ids, E)
    want = np.argsort(key, kind="stable")[:n]
    got = order[:n]
    assert np.array_equal(got, want), f"order differs from the stable argsort at {np.nonzero(got != want)[0][:8].tolist()} of {n}"


# ------------------------------------------------------------------ silu

def silu_mul_ref(gate_up):
    """(want, bound) float64 [..., D] of silu(gate) * up for gate_up [..., 2 D] fp16 = [gate | up]"""
    gu = np.asarray(gate_up)
    assert gu.dtype == np.float16
    D = gu.shape[-1] // 2
    g, u = gu[..., :D].astype(np.float64), gu[..., D:].astype(np.float64)
    with np.errstate(over="ignore"):
        want = g / (1.0 + np.exp(-g)) * u
    return want, ulp16(want) / 2 * (1.0 + 2.0 ** -10) + gamma(SILU_N) * np.abs(want) * 1.01


def check_silu(gate_up, got, what=""):
    """the finite / non-finite pattern equals that of fp16(want), infinities carry want's sign, finite values within the bound;
    returns the largest err / bound"""
    want, bnd = silu_mul_ref(gate_up)
    got = np.asarray(got)
    assert got.dtype == np.float16 and got.shape == want.shape, (what, got.dtype, got.shape)
    with np.errstate(over="ignore"):
        w16 = want.astype(np.float16)
    fin = np.isfinite(w16)
    assert np.array_equal(np.isfinite(got), fin), f"{what}: finite / non-finite pattern differs at {np.argwhere(np.isfinite(got) != fin)[:4].tolist()}"
    assert np.array_equal(got[~fin], w16[~fin]), f"{what}: an overflow with the wrong sign"
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    bad = ~(err <= bnd[fin])
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} outside the derived bound; first: got {got[fin][i]!r}, want {want[fin][i]!r}, "
                             f"err {err[i]:.3g} = {err[i] / bnd[fin][i]:.3g} x bound")
    return float((err / bnd[fin]).max()) if err.size else 0.0


def silu_input(rows, D, seed):
    """gates drawn over [-20, 20], ups ~ 3 N(0, 1), with special gates spliced into the first row: 0, -0, 65504 (x 0.5: finite;
    x 1: exactly the largest fp16; x 2 and x -2: overflow, when D has the room), -65504 (silu = -0), 1e-4, -20"""
    rng = np.random.default_rng([seed, rows, D])
    gu = np.empty((rows, 2 * D), np.float16)
    gu[:, :D] = rng.uniform(-20.0, 20.0, (rows, D)).astype(np.float16)
    gu[:, D:] = (3.0 * rng.standard_normal((rows, D))).astype(np.float16)
    gates = [0.0, -0.0, 65504.0, -65504.0, 1e-4, -20.0, 65504.0, 65504.0, 65504.0]
    ups = [None, None, 0.5, None, None, None, 1.0, 2.0, -2.0]
    for i, (g, u) in enumerate(zip(gates, ups)):
        if i < D:
            gu[0, i] = g
            if u is not None:
                gu[0, D + i] = u
    return gu


# ------------------------------------------------------------------ case families

def logits_for_choice(choice, E, rng):
    """decidable logits whose reference routing is exactly `choice` [T, k] (distinct experts per row, in selection order): the
    j-th choice gets 8 - 0.5 j, every other expert -1 - 0.25 {0..8} (ties among the unchosen are harmless)"""
    choice = np.asarray(choice)
    T, k = choice.shape
    lg = (-1.0 - 0.25 * rng.integers(0, 9, (T, E))).astype(np.float32)
    for j in range(k):
        lg[np.arange(T), choice[:, j]] = np.float32(8.0 - 0.5 * j)
    return lg


def deal(counts, T, k, rng):
    """`choice` [T, k] with expert e chosen counts[e] times (sum = T k, every count <= T), k distinct experts per token: the
    experts' runs are dealt round the tokens, so a run of at most T pairs never meets a token twice; the slot order is shuffled"""
    counts = np.asarray(counts)
    assert counts.sum() == T * k and counts.max() <= T and counts.min() >= 0
    labels = np.repeat(np.arange(counts.size), counts)
    start = int(rng.integers(0, T))
    choice = np.empty((T, k), np.int64)
    fill = np.zeros(T, np.int64)
    for i, e in enumerate(labels):
        t = (start + i) % T
        choice[t, fill[t]] = e
        fill[t] += 1
    assert (fill == k).all()
    for t in range(T):
        rng.shuffle(choice[t])
        assert len(set(choice[t].tolist())) == k
    return choice


def _local_counts(kind, T, E, k, block, e0, nl, rng):
    """pair counts per expert with the LOCAL experts' counts = 1 (mod block) or multiples of the block, or None"""
    P = T * k
    foreign = E - nl
    if kind == "one_mod_block":
        base, unit_cap = 1, (T - 1) // block
    else:
        base, unit_cap = 0, T // block
    if base > T:
        return None
    # units of `block` pairs on top of the base: as many as fit, leaving the foreign experts what they can hold (<= T each)
    lo = P - nl * base - foreign * T           # pairs the local experts must take beyond their base
    hi = min(P - nl * base, nl * unit_cap * block)
    if foreign == 0:
        if hi < 0 or (P - nl * base) % block or P - nl * base > nl * unit_cap * block:
            return None
        units = (P - nl * base) // block
    else:
        if hi < 0:
            return None
        units_lo = max(0, -(-lo // block))
        units_hi = hi // block
        if units_lo > units_hi:
            return None
        units = int(rng.integers(units_lo, units_hi + 1)) if kind == "one_mod_block" else units_hi
        if kind == "multiple" and units == 0:
            return None  # (every local count 0 is `empties`' business)
    local = np.full(nl, base, np.int64)
    for _ in range(units):
        free = np.nonzero(local + block <= T)[0]
        local[free[int(rng.integers(0, free.size))]] += block
    counts = np.zeros(E, np.int64)
    counts[e0:e0 + nl] = local
    rest = P - int(local.sum())
    others = [e for e in range(E) if not e0 <= e < e0 + nl]
    for i in range(rest):  # spread evenly: never more than T each (rest <= foreign * T)
        counts[others[i % len(others)]] += 1
    return counts if counts.max() <= T else None


def build(family, T, E, k, seed, block=8, e0=0, nl=None, second=None, top=None):
    """fp32 logits [T, E] of `family` (module docstring), or None where (T, E, k[, block, e0, nl]) cannot carry it.  `second`:
    spread's runner-up value; `top`: crowded's two experts.  "spread_distinct" is spread with no two equal logits in a row."""
    nl = E - e0 if nl is None else nl
    rng = np.random.default_rng([seed, T, E, k, block, e0, nl, len(family), ord(family[0])])
    f32 = np.float32
    if family == "ties":
        return (0.25 * rng.integers(-4, 5, (T, E))).astype(f32)
    if family == "all_equal":
        return np.full((T, E), 0.25 * float(rng.integers(-8, 9)), f32)
    if family == "near":
        return (1.0 + rng.integers(0, 3, (T, E)) * 2.0 ** -12).astype(f32)
    if family in ("spread", "spread_distinct"):
        if family == "spread_distinct":
            if E > 320:
                return None
            steps = np.stack([rng.permutation(320)[:E] + 1 for _ in range(T)])
        else:
            steps = rng.integers(1, 321, (T, E))
        lg = (-0.25 * steps).astype(f32)
        if second is not None and E >= 2:
            lg = np.minimum(lg, f32(second - 0.25))
        win = rng.integers(0, E, T)
        if second is not None and E >= 2:
            lg[np.arange(T), (win + 1 + rng.integers(0, E - 1, T)) % E] = f32(second)
        lg[np.arange(T), win] = 0.0
        return lg
    if family in ("big", "neg"):
        sign = 1.0 if family == "big" else -1.0
        if E > 81:
            return None
        steps = np.stack([rng.permutation(81)[:E] - 40 for _ in range(T)])  # distinct multiples of 0.5 in [-20, 20]
        return (sign * 30000.0 + 0.5 * steps).astype(f32)
    if family == "crowded":
        if E < 2 or k < 2:
            return None
        a, b = top if top is not None else (int(rng.integers(0, E)), None)
        if b is None:
            b = (a + 1 + int(rng.integers(0, E - 1))) % E
        others = [e for e in range(E) if e not in (a, b)]
        lg = np.empty((T, E), f32)
        for t in range(T):  # distinct values below the runner-up: -2, -2.25, ... in a random order per token
            lg[t, others] = -2.0 - 0.25 * rng.permutation(len(others))
        lg[:, a] = 0.0
        lg[:, b] = f32(np.log(0.3 / 0.7))
        return lg
    if family in ("one_mod_block", "multiple"):
        if block < 1:
            return None
        counts = _local_counts(family, T, E, k, block, e0, nl, rng)
        if counts is None:
            return None
        lg = logits_for_choice(deal(counts, T, k, rng), E, rng)
        c = np.bincount(route_ref(lg, k, True)[1].reshape(-1), minlength=E)[e0:e0 + nl]
        assert ((c % block == 1) if family == "one_mod_block" else (c % block == 0)).all()
        return lg
    if family == "empties":
        if k > 2 or (k == 2 and E < 2):
            return None
        pair = np.array([0, E - 1])
        choice = np.stack([rng.permutation(pair)[:k] for _ in range(T)])
        return logits_for_choice(choice, E, rng)
    raise ValueError(family)


def cases(T, E, k, seed=0, block=8, e0=0, nl=None, families=FAMILIES):
    """[(family, logits)] over the families the shape can carry"""
    out = []
    for fam in families:
        lg = build(fam, T, E, k, seed, block=block if block > 0 else 8, e0=e0, nl=nl)
        if lg is not None:
            out.append((fam, lg))
    return out


# the shapes the GPU tests of the route kernel run (T = 8 | 9: the one-block / two-launch edge)
ROUTE_SHAPES = [(1, 8, 2), (8, 8, 2), (9, 8, 2), (37, 8, 2), (8, 64, 8), (9, 64, 8), (5, 33, 4), (4, 63, 1), (3, 1, 1), (6, 5, 5), (130, 16, 4)]
ROUTE_BLOCKS = (0, 8, 16, 4)
LOCAL_FORMS = [(8, 2, 2, 3), (8, 2, 6, 2), (64, 8, 0, 1), (64, 8, 63, 1)]  # (E, k, e0, nl), at T = 8 and T = 9
