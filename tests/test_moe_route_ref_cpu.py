"""tests/moe_route_ref.py proves itself on the CPU: float32 numpy restatements of awq_moe_route_kernel's routing (its order of
operations, butterflies included), of its alignment pass (one thread per expert walking the pairs) and of awq_moe_sort_kernel
(chunks of 1024, per-wave ranks) pass every checker on every family at the shapes the GPU tests run; each named defect fails the
checker on the family named for it; every case built is decidable; and the reference agrees with the ones the suite already has
(ops.fused_topk, ops.moe_align_block_size, ep.local_routing on CPU tensors, oracle.moe_forward)."""
import numpy as np
import pytest
import torch

import moe_route_ref as mr

F32 = np.float32
LANES = np.arange(64)
BLOCK_T = (6, 7, 32, 33, 191, 192)  # tests/test_gpu_moe_block_routes.py: E = 8, top-2


# ------------------------------------------------------------------ float32 restatements of the kernels

def kernel_route(lg, k, renorm, defect=None):
    """elementwise.hip:73-106, one token at a time: lane e holds expert e's logit, lanes past E hold -inf / -3"""
    T, E = lg.shape
    w, ids = np.empty((T, k), F32), np.empty((T, k), np.int32)
    for t in range(T):
        row = np.full(64, -np.inf, F32)
        row[:E] = lg[t]
        mx = row.copy()
        o = 32
        while o:
            mx = np.maximum(mx, mx[LANES ^ o])
            o //= 2
        if defect == "no_max":
            mx = np.zeros(64, F32)
        with np.errstate(all="ignore"):
            v = np.exp(row - mx)
        assert v.dtype == F32
        v[E:] = -3.0
        s = F32(0.0)
        with np.errstate(all="ignore"):
            for e in range(E):
                s = F32(s + v[e])
        picked, vals = [], []
        for _ in range(k):
            bv, best = v.copy(), LANES.copy()
            o = 32
            while o:
                ov, oi = bv[LANES ^ o], best[LANES ^ o]
                tie = (oi > best) if defect == "highest_index" else (oi < best)
                take = (ov > bv) | ((ov == bv) & tie)
                bv, best = np.where(take, ov, bv), np.where(take, oi, best)
                o //= 2
            assert (best == best[0]).all() and (bv == bv[0]).all()  # every lane ends with the same winner
            v[best[0]] = -2.0
            picked.append(int(best[0]))
            vals.append(F32(bv[0]))
        with np.errstate(all="ignore"):
            if defect == "topk_denominator":
                s = F32(0.0)
                for x in vals:
                    s = F32(s + x)
            inv = F32(1.0) / s
            wsum, out = F32(0.0), []
            for x in vals:
                wj = F32(x * inv)
                wsum = F32(wsum + wj)
                out.append(wj)
            if defect == "renorm_all":
                wsum = F32(s * inv)
            w[t] = [F32(x / wsum) for x in out] if renorm else out
        ids[t] = picked
    if defect == "swap":
        w[:, [0, 1]] = w[:, [1, 0]]
    return w, ids


def kernel_align(ids, E, block, e0=0, nl=None, defect=None):
    """elementwise.hip:111-133 on the id table phase 1 wrote"""
    flat = np.asarray(ids).reshape(-1)
    nl = E - e0 if nl is None else nl
    P = flat.size
    counts = np.array([(flat == e0 + e).sum() for e in range(nl)])
    pad_start = np.zeros(nl + 1, np.int64)
    for e in range(nl):
        blocks = (counts[e] + block - 1) // block
        if defect == "block_for_empty":
            blocks = max(blocks, 1)
        pad_start[e + 1] = pad_start[e] + blocks * block
    npad = int(pad_start[nl])
    cap_sorted, cap_blocks = P + nl * (block - 1), P + nl
    sorted_ids = np.full(max(cap_sorted, npad), P - 1 if defect == "sentinel" else P, np.int32)
    expert_ids = np.empty(cap_blocks, np.int32)
    for b in range(cap_blocks):
        e = 0
        while e < nl - 1 and b * block >= pad_start[e + 1]:
            e += 1
        expert_ids[b] = e + (e0 if defect == "absolute" else 0)
    for e in range(nl):  # one thread per (local) expert
        pos = pad_start[e]
        for p in (range(P - 1, -1, -1) if defect == "descending" else range(P)):
            if flat[p] == e0 + e:
                sorted_ids[pos] = p
                pos += 1
    return sorted_ids[:cap_sorted], expert_ids, np.array([npad], np.int32)


def kernel_sort(ids, E, defect=None):
    """elementwise.hip:167-213: a histogram, then per chunk of 1024 the rank of a pair = its expert's pairs in earlier waves of
    the chunk + in earlier lanes of its wave, on top of the expert's cursor"""
    ids = np.asarray(ids).reshape(-1)
    P = ids.size
    ok = (ids >= 0) & (ids < E)
    cnt = np.bincount(ids[ok], minlength=E)
    seg = np.zeros(E + 1, np.int32)
    seg[1:] = np.cumsum(cnt)
    cursor = seg[:E].astype(np.int64).copy()
    order = np.full(P, -7, np.int32)  # (slots past seg[E] are never written)
    for c0 in range(0, P, 1024):
        chunk = np.full(1024, -1, np.int64)
        chunk[: min(1024, P - c0)] = ids[c0:c0 + 1024]
        valid = (chunk >= 0) & (chunk < E)
        wcnt = np.zeros((16, E), np.int64)
        rank = np.zeros(1024, np.int64)
        for wv in range(16):
            sl = slice(64 * wv, 64 * wv + 64)
            for x in np.unique(chunk[sl][valid[sl]]):
                m = valid[sl] & (chunk[sl] == x)
                wcnt[wv, x] = m.sum()
                rank[sl][m] = np.cumsum(m)[m] - 1
        for i in np.nonzero(valid)[0]:
            e, wv = chunk[i], i // 64
            order[cursor[e] + wcnt[:wv, e].sum() + rank[i]] = c0 + i
        if defect != "cursor":
            cursor += wcnt.sum(0)
    return order, seg


def kernel_silu(gu, defect=None):
    """awq_device.h awq_silu_mul_f32: expf(-g), 1 + e, g / d, q * u in fp32, one rounding to fp16"""
    D = gu.shape[-1] // 2
    g, u = gu[..., :D].astype(F32), gu[..., D:].astype(F32)
    if defect == "halves_swapped":
        g, u = u, g
    with np.errstate(all="ignore"):
        q = g / (F32(1.0) + np.exp(-g))
        if defect == "fp16_silu":
            q = q.astype(np.float16).astype(F32)
        return (q * u).astype(np.float16)


# ------------------------------------------------------------------ the cases are decidable and every family is carried

def route_cases():
    """every (what, logits, k, block, e0, nl) the GPU route tests build"""
    for T, E, k in mr.ROUTE_SHAPES:
        for block in mr.ROUTE_BLOCKS:
            for fam, lg in mr.cases(T, E, k, seed=T + E, block=block):
                yield f"{fam} T{T} E{E} k{k} block{block}", fam, lg, k, block, 0, E
    for E, k, e0, nl in mr.LOCAL_FORMS:
        for T in (8, 9):
            for block in (8, 16):
                for fam, lg in mr.cases(T, E, k, seed=T + E, block=block, e0=e0, nl=nl):
                    yield f"{fam} T{T} E{E} k{k} block{block} local {e0}+{nl}", fam, lg, k, block, e0, nl


ROUTE_CASES = list(route_cases())


def test_every_case_is_decidable_and_every_family_is_carried():
    seen = {}
    for what, fam, lg, k, block, e0, nl in ROUTE_CASES:
        assert lg.dtype == F32 and mr.decidable(lg), what
        seen.setdefault(fam, set()).add((lg.shape, block, e0, nl))
    assert set(seen) == set(mr.FAMILIES)
    # the full-capacity case and the no-padding case exist on both sides of the T = 8 | 9 edge, globally and locally
    for fam in ("one_mod_block", "multiple"):
        glob = {s[0] for s, b, e0, nl in seen[fam] if nl == s[1] and b > 0}
        assert any(T <= 8 for T in glob) and any(T > 8 for T in glob), (fam, glob)
        assert any(nl != s[1] for s, b, e0, nl in seen[fam]), fam
    for T in BLOCK_T:
        for fam in ("crowded", "all_equal", "empties"):
            assert mr.decidable(mr.build(fam, T, 8, 2, T))
        assert mr.decidable(mr.build("spread", T, 8, 2, T, second=-60.0))
    assert all(mr.build("one_mod_block", T, 8, 2, T, block=8) is not None for T in (32, 192))
    assert all(mr.build("multiple", T, 8, 2, T, block=8) is not None for T in (32, 192))


def test_one_mod_block_fills_the_capacity_and_multiple_has_no_padding(oracle):
    for what, fam, lg, k, block, e0, nl in ROUTE_CASES:
        if block == 0 or fam not in ("one_mod_block", "multiple"):
            continue
        assert mr.decidable(lg), what
        ids = mr.route_ref(lg, k, True)[1].reshape(-1)
        owned = (ids >= e0) & (ids < e0 + nl)
        s, e, n = oracle.moe_align(np.where(owned, ids - e0, nl), nl, block)
        if fam == "one_mod_block":
            assert n == int(owned.sum()) + nl * (block - 1), what
            if nl == lg.shape[1]:
                assert n == s.size and s[n - block] != ids.size, what  # the last block of the capacity is in use
        else:
            assert n == int(owned.sum()) and (s[:n] != ids.size).all(), what


def test_decidable_refuses_close_wide_and_non_finite_rows():
    ok = np.array([[0.0, 1.0, 1.0, -79.0]], F32)
    assert mr.decidable(ok)
    for bad in ([[0.0, 2.0 ** -13]], [[0.0, -80.5]], [[0.0, np.nan]], [[0.0, np.inf]], [[0.0, -0.0]], [[1.0, 1.0 + 2.0 ** -13]]):
        assert not mr.decidable(np.array(bad, F32)), bad
    assert not mr.decidable(ok.astype(np.float64))


# ------------------------------------------------------------------ the restatements pass

@pytest.mark.parametrize("renorm", [True, False])
def test_route_restatement_passes_on_every_case(renorm):
    worst = {}
    for what, fam, lg, k, block, e0, nl in ROUTE_CASES:
        if block not in (0, 8):
            continue  # (the routing does not depend on the block; the families built for a block do)
        assert mr.decidable(lg), what
        w, ids = kernel_route(lg, k, renorm)
        worst[fam] = max(worst.get(fam, 0.0), mr.check_route(lg, k, renorm, w, ids, what))
    print(f"float32 restatement, renorm={renorm}: max err / bound", {f: round(r, 3) for f, r in worst.items()})
    assert set(worst) == set(mr.FAMILIES)


def test_alignment_restatement_passes_on_every_case():
    n = 0
    for what, fam, lg, k, block, e0, nl in ROUTE_CASES:
        if block == 0:
            continue
        assert mr.decidable(lg), what
        ids = mr.route_ref(lg, k, True)[1]
        mr.check_alignment(ids, lg.shape[1], block, *kernel_align(ids, lg.shape[1], block, e0, nl), e0=e0, nl=nl)
        n += 1
    assert n > 100


def sort_cases():
    """every (what, ids, E) the GPU sort test builds, but for the routed one"""
    for E in (1, 8, 64):
        for P in (1, 1023, 1024, 1025, 2049):
            yield f"P{P} all on expert {E - 1 if E == 64 else 0} of {E}", np.full(P, 63 if E == 64 else 0, np.int32), E
        foreign = np.where(np.arange(1500) % 2 == 0, -1, E + 3).astype(np.int32)
        yield f"all foreign E{E}", foreign, E
        alt = np.where(np.arange(2049) % 2 == 0, np.arange(2049) % E, foreign[0]).astype(np.int32)
        alt[3::4] = E + 3
        yield f"alternating E{E}", alt, E


def test_sort_restatement_passes():
    for what, ids, E in sort_cases():
        order, seg = kernel_sort(ids, E)
        mr.check_sort(ids, E, order, seg)
        if "foreign" in what:
            assert not seg.any()
    lg = mr.build("crowded", 700, 8, 2, 1)
    assert mr.decidable(lg)
    ids = mr.route_ref(lg, 2, True)[1]
    mr.check_sort(ids, 8, *kernel_sort(ids, 8))


def test_silu_restatement_passes_and_defects_fail():
    for rows, D in ((1, 8), (37, 1408)):
        gu = mr.silu_input(rows, D, seed=4)
        r = mr.check_silu(gu, kernel_silu(gu))
        print(f"silu float32 restatement {rows} x {D}: max err / bound {r:.3f}")
        for defect in ("halves_swapped", "fp16_silu"):
            if D > 8 or defect == "halves_swapped":
                with pytest.raises(AssertionError):
                    mr.check_silu(gu, kernel_silu(gu, defect))
    gu = mr.silu_input(1, 16, seed=1)
    want = mr.silu_mul_ref(gu)[0][0]
    assert want[2] == 32752.0 and want[6] == 65504.0 and want[7] > 1e5 and want[8] < -1e5 and want[3] == 0.0
    got = kernel_silu(gu)
    got[0, 7] = -got[0, 7]
    with pytest.raises(AssertionError, match="wrong sign"):
        mr.check_silu(gu, got)


# ------------------------------------------------------------------ the named defects fail

def _case(fam, T, E, k, **kw):
    lg = mr.build(fam, T, E, k, 5, **kw)
    assert lg is not None and mr.decidable(lg), fam
    return lg


@pytest.mark.parametrize("defect,fam,renorm", [
    ("highest_index", "ties", True), ("highest_index", "all_equal", True), ("no_max", "big", True),
    ("topk_denominator", "spread", False), ("renorm_all", "crowded", True), ("swap", "crowded", True)])
@pytest.mark.parametrize("T,E,k", [(9, 8, 2), (8, 64, 8), (130, 16, 4)])
def test_route_defects_fail(defect, fam, renorm, T, E, k):
    lg = _case(fam, T, E, k)
    w, ids = kernel_route(lg, k, renorm)
    mr.check_route(lg, k, renorm, w, ids)
    w, ids = kernel_route(lg, k, renorm, defect)
    with pytest.raises(AssertionError):
        mr.check_route(lg, k, renorm, w, ids)


@pytest.mark.parametrize("defect,fam,T,E,k,block,e0,nl", [
    ("sentinel", "one_mod_block", 8, 8, 2, 4, 0, 8), ("sentinel", "one_mod_block", 9, 64, 8, 8, 0, 64),
    ("block_for_empty", "empties", 9, 8, 2, 8, 0, 8), ("block_for_empty", "empties", 4, 63, 1, 16, 0, 63),
    ("descending", "crowded", 9, 8, 2, 8, 0, 8), ("descending", "crowded", 8, 64, 8, 16, 0, 64),
    ("absolute", "crowded", 8, 8, 2, 8, 2, 3), ("absolute", "one_mod_block", 9, 64, 8, 8, 63, 1), ("absolute", "one_mod_block", 9, 8, 2, 16, 6, 2)])
def test_alignment_defects_fail(defect, fam, T, E, k, block, e0, nl):
    lg = _case(fam, T, E, k, block=block, e0=e0, nl=nl, top=(3, 4) if fam == "crowded" and e0 else None)
    ids = mr.route_ref(lg, k, True)[1]
    mr.check_alignment(ids, E, block, *kernel_align(ids, E, block, e0, nl), e0=e0, nl=nl)
    with pytest.raises(AssertionError):
        mr.check_alignment(ids, E, block, *kernel_align(ids, E, block, e0, nl, defect), e0=e0, nl=nl)


def test_sort_defect_cursor_not_advanced_fails():
    ids = np.zeros(2049, np.int32)
    mr.check_sort(ids, 1, *kernel_sort(ids, 1))
    with pytest.raises(AssertionError):
        mr.check_sort(ids, 1, *kernel_sort(ids, 1, "cursor"))
    with pytest.raises(AssertionError):  # (and seg is looked at: the counts of two experts exchanged)
        order, seg = kernel_sort(np.array([0, 1, 1], np.int32), 2)
        mr.check_sort(np.array([0, 1, 1], np.int32), 2, order, np.array([0, 2, 3], np.int32))


# ------------------------------------------------------------------ agreement with the references the suite already has

def test_fused_topk_agrees_on_the_families_without_ties():
    from autoawq_amd import ops

    n = 0
    for T, E, k in mr.ROUTE_SHAPES:
        for fam in mr.NO_TIES:
            lg = mr.build(fam, T, E, k, T + E)
            if lg is None:
                continue
            assert mr.decidable(lg) and all(len(set(r.tolist())) == E for r in lg), fam
            for renorm in (True, False):
                w, ids = ops.fused_topk(torch.from_numpy(lg), k, renorm)
                mr.check_route(lg, k, renorm, w.numpy(), ids.numpy(), f"fused_topk {fam} T{T} E{E} k{k}")
                n += 1
    assert n > 40


def test_torch_alignment_and_local_routing_pass_on_every_case():
    from autoawq_amd import ep, ops

    for what, fam, lg, k, block, e0, nl in ROUTE_CASES:
        if block == 0:
            continue
        assert mr.decidable(lg), what
        E = lg.shape[1]
        ids = mr.route_ref(lg, k, True)[1]
        if nl == E:
            s, e, n = ops.moe_align_block_size(torch.from_numpy(ids), block, E)
            mr.check_alignment(ids, E, block, s.numpy(), e.numpy(), n.numpy(), e0=0, nl=E)
            e0s = [(0, E)] if E == 1 else [(0, (E + 1) // 2), ((E + 1) // 2, E - (E + 1) // 2)]
        else:
            e0s = [(e0, nl)]
        for a, m in e0s:
            s, e, n, owned = ep.local_routing(torch.from_numpy(ids), a, m, block)
            assert np.array_equal(owned.numpy(), (ids >= a) & (ids < a + m))
            mr.check_alignment(ids, E, block, s.numpy(), e.numpy(), n.numpy(), e0=a, nl=m, parked=True)


def test_parked_bucket_is_checked():
    from autoawq_amd import ep

    lg = mr.build("ties", 9, 8, 2, 3)
    assert mr.decidable(lg)
    ids = mr.route_ref(lg, 2, True)[1]
    s, e, n, _ = ep.local_routing(torch.from_numpy(ids), 2, 3, 8)
    s = s.numpy().copy()
    mr.check_alignment(ids, 8, 8, s, e.numpy(), n.numpy(), e0=2, nl=3, parked=True)
    with pytest.raises(AssertionError):  # without the allowance the parked pairs are slots past npad that are no sentinel
        mr.check_alignment(ids, 8, 8, s, e.numpy(), n.numpy(), e0=2, nl=3)
    s[int(n)], s[int(n) + 1] = s[int(n) + 1], s[int(n)]
    with pytest.raises(AssertionError):
        mr.check_alignment(ids, 8, 8, s, e.numpy(), n.numpy(), e0=2, nl=3, parked=True)


def _tiny_stacks(E, H, I, g, seed):
    rng = np.random.default_rng(seed)

    def one(K, N):
        return dict(qweight=rng.integers(-2 ** 31, 2 ** 31, (E, K, N // 8)).astype(np.int32),
                    qzeros=rng.integers(-2 ** 31, 2 ** 31, (E, K // g, N // 8)).astype(np.int32),
                    scales=(rng.random((E, K // g, N)) * 0.02 + 0.005).astype(np.float16))
    return one(H, 2 * I), one(I, H)


@pytest.mark.parametrize("T,E,k", [(9, 8, 2), (6, 5, 5), (5, 33, 4), (8, 64, 8)])
def test_route_ref_agrees_with_the_oracles_moe_block(oracle, T, E, k):
    """oracle.moe_forward picks by descending float32 PROBABILITY with a stable sort: on decidable logits that is the reference's
    choice, ties included, and its renormalised fp32 weights are within the kernel's bound of the float64 ones"""
    w1, w2 = _tiny_stacks(E, 128, 128, 128, E)
    x = np.random.default_rng(T).standard_normal((T, 128)).astype(np.float16)
    for fam, lg in mr.cases(T, E, k, seed=11):
        assert mr.decidable(lg)
        _, ids, wt = oracle.moe_forward(x, lg, w1, w2, k, 128)
        mr.check_route(lg, k, True, wt, ids, f"oracle.moe_forward {fam}")
