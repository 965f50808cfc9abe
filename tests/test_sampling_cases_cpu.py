"""tests/sampling_cases.py without a GPU: every case is the designed one and meets the conditions its witnesses need, and
check_draws refuses a sampler whose kept set is one value too large or one value too small -- the proof that a kernel whose
threshold is off by one step fails tests/test_gpu_sampling_kept_set.py."""
import math

import numpy as np
import pytest

import penalty_ref as pref
import sampling_cases as sc
import sampling_ref as ref
from test_sampling_cpu import _hf_kept

ALL = sc.CASES + sc.PROC_CASES
ids = [c.name for c in ALL]
# case -> (key of the boundary value = the threshold the kernel has to find, key of the first excluded value), by design
THRESHOLDS = {
    "k_on_edge_lo00": (0xC100, 0xC0FF), "k_below_edge_loFF": (0xC0FF, 0xC0FE), "k_above_edge_lo01": (0xC101, 0xC100),
    "k_mid_bin": (0xC180, 0xC17F), "k_in_bin_of_max": (0xC127, 0xC126),
    "zero_k_cuts_group": (0x8000, 0x7FFE), "zero_k_above": (0x8001, 0x8000), "zero_k_exact": (0x8000, 0x7FFE),
    "zero_k_below": (0x7FFE, 0x7FFD),
    "bottom_k_is_count": (0x0400, None), "bottom_k_count_plus_1": (0x0400, None), "bottom_k_count_minus_1": (0x0401, 0x0400),
    "bottom_k_is_V": (0x0400, None),
    "tie_group_top_k": (0xBC00, 0xBBFF), "tie_group_top_p": (0xBC00, 0xBBFF),
    "p_top_bin": (0xC107, 0xC106), "p_between_bins": (0xC1FC, 0xC1FB), "p_in_k_bin_above": (0xC0FD, 0xC0FC),
    "p_equals_k": (0xC0FE, 0xC0FD), "p_lo00": (0xC100, 0xC0FF), "p_loFF": (0xC0FF, 0xC0FE), "p_cold_zero_masses": (0xC100, 0xB533),
    "k_p_T_together": (0xC0FF, 0xC0FE),
    "penalty_moves_down": (0xBE27, 0xBE10), "penalty_moves_up": (0x4940, 0x4900), "min_new_hides_max": (0xC100, 0xC0FF),
}


def test_key_space_restates_key16():
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    v = bits.view(np.float16).astype(np.float64)
    k = sc.key16(bits).astype(np.int64)
    ok = ~np.isnan(v)
    order = np.argsort(v[ok], kind="stable")
    assert (np.diff(k[ok][order]) >= 0).all()                                   # monotone ...
    assert ((np.diff(k[ok][order]) == 0) == (np.diff(v[ok][order]) == 0)).all()  # ... and equal keys are equal values
    assert sc.key16(0x8000) == sc.key16(0x0000) == 0x8000                       # -0 folded into +0
    assert sc.key16(np.float16(-65504).view(np.uint16)) == 0x0400 and sc.key16(np.float16(-np.inf).view(np.uint16)) == 0x03FF
    assert sc.key16(np.float16(65504).view(np.uint16)) == 0xFBFF
    keys = np.array([k for k in range(0x0400, 0xFC00) if k != 0x7FFF])
    assert np.array_equal(sc.key16(sc.bits_of_key(keys)), keys)                 # the inverse, on every finite key
    assert sc.bits_of_key(sc.NEG_ZERO) == 0x8000
    assert sc.value_of_key(0xBC00) == 1.0 and sc.value_of_key(0x43FF) == -1.0


def test_schedule_gumbel_is_the_restatement_row_by_row():
    g = sc.schedule_gumbel(sc.SEED, 1, sc.ROWS, sc.V_C)
    for r in (0, 1, 77, sc.ROWS - 1):
        assert np.array_equal(g[r], ref.gumbel(sc.SEED, 1, r, sc.V_C))


def _bins(c):
    """high bytes of the maximum, of the top-k threshold (bin 4 with top-k off) and of the top-p threshold"""
    kth = np.sort(c.logits.astype(np.float64))[-c.top_k] if c.top_k else -65504.0
    return tuple(int(sc.keys_of(np.float16(v))) >> 8 for v in (c.logits.max(), kth, sc.draws(c).boundary))


def test_the_cases_the_issue_lists_are_there():
    assert set(THRESHOLDS) == set(sc.BY_NAME)
    keys = {c.name: {k for k, _ in c.groups} for c in ALL}
    for V in (sc.V_A, sc.V_B, sc.V_C):
        assert len(sc.cases_of(V)) % 3 and 4100 <= V <= 6200    # (the rows form makes every third row greedy: no case always greedy)
    assert sc.V_C % 8 and all(c.strided == (c.V == sc.V_C) for c in ALL)
    for c in ALL:
        cand = np.concatenate([i for _, i in c.groups] + [np.array(c.eos, dtype=np.int64)])
        assert {0, 2047, 2048, c.V - 1} <= set(cand.tolist()), c.name
        assert {int(i) // 2048 for i in cand} == set(range((c.V + 2047) // 2048)), c.name
        assert len(c.groups) <= 40 and len(cand) < c.V // 8, c.name
        rest = np.delete(c.raw, cand)
        low = c.logits[cand].astype(np.float64)
        assert (rest == rest[0]).all() and float(rest[0]) < low[np.isfinite(low)].min() - 20, c.name   # the filler: one far lower value
        d = sc.draws(c)
        b, e = THRESHOLDS[c.name]
        assert int(sc.keys_of(np.float16(d.boundary))) == b, c.name
        assert (d.excluded is None) == (e is None) and (e is None or int(sc.keys_of(np.float16(d.excluded))) == e), c.name
    by = sc.BY_NAME
    assert {k >> 8 for k in keys["k_in_bin_of_max"]} == {0xC1}
    assert len({k >> 8 for k in keys["k_mid_bin"]}) >= 5
    z = by["zero_k_cuts_group"]
    assert {0x0000, 0x8000, 0x0001, 0x8001} <= set(z.raw.view(np.uint16).tolist())          # +0, -0, +-subnormal
    assert (z.raw[z.kept].view(np.uint16) == 0x8000).sum() == 2 and (z.raw[z.kept].view(np.uint16) == 0).sum() == 2
    for name in ("bottom_k_is_count", "bottom_k_count_plus_1", "bottom_k_count_minus_1", "bottom_k_is_V"):
        c = by[name]
        n = int(np.isfinite(c.raw).sum())
        assert np.isneginf(c.raw).sum() == c.V - n and c.raw[np.isfinite(c.raw)].max() < 0 and -65504.0 in c.raw
        assert c.top_k == {"bottom_k_is_count": n, "bottom_k_count_plus_1": n + 1, "bottom_k_count_minus_1": n - 1, "bottom_k_is_V": c.V}[name]
    for name in ("tie_group_top_k", "tie_group_top_p"):
        c = by[name]
        grp = [i for k, i in c.groups if len(i) >= 290][0]
        assert {int(i) // 2048 for i in grp} == {0, 1, 2, 3} and set(grp.tolist()) <= set(c.kept.tolist())
    above = np.sort(by["tie_group_top_k"].raw.astype(np.float64))[::-1]
    assert above[5] == above[304] == 1.0 and 5 < by["tie_group_top_k"].top_k < 305      # k cuts through the group
    t, k, p = _bins(by["p_top_bin"])
    assert t == p
    t, k, p = _bins(by["p_between_bins"])
    assert t > p > k
    c = by["p_in_k_bin_above"]
    t, k, p = _bins(c)
    assert p == k and sc.draws(c).boundary > np.sort(c.logits.astype(np.float64))[-c.top_k]
    c = by["p_equals_k"]
    assert sc.draws(c).boundary == np.sort(c.logits.astype(np.float64))[-c.top_k] and c.top_p < 1
    assert {c.temperature for c in sc.CASES if c.top_p < 1} >= {0.25, 1.0, 2.0, 0.05}
    c = by["p_cold_zero_masses"]
    x = c.logits.astype(np.float32)
    arg = (x - x.max()) / np.float32(c.temperature)
    assert c.top_p == 0.999 and ((arg < -31) == ~sc.draws(c).keep).all() and (arg[np.isfinite(arg)] < -31).sum() > 6
    c = by["k_p_T_together"]
    assert c.top_k and c.top_p < 1 and c.temperature != 1


@pytest.mark.parametrize("case", ALL, ids=ids)
def test_case_is_sound(case):
    d = sc.draws(case)
    assert np.array_equal(np.flatnonzero(d.keep), case.kept)                    # the designed set, stated index by index
    assert len({k for k, i in case.groups if set(i.tolist()) <= set(case.kept.tolist())}) >= 2
    assert int(d.in_w.sum()) >= sc.MIN_WITNESSES, d.in_w.sum()
    if d.excluded is not None and not case.no_out:
        assert int(d.out_w.sum()) >= sc.MIN_WITNESSES, d.out_w.sum()
    if case.no_out:
        # the one case whose first excluded value cannot win: its share of the kept mass is below e^-45 (sampling_cases.py)
        x = case.logits.astype(np.float64) / case.temperature
        assert d.excluded is not None and d.excluded / case.temperature - x.max() < -45.0
    if case.top_p < 1.0:
        assert sc.top_p_margin_holds(case), sc.top_p_sides(case)
    wins = sc.decisive_wins(case)
    assert min(wins.values()) >= 1, {hex(k): v for k, v in wins.items()}
    assert d.want.shape == (len(case.ts), case.rows) and case.rows >= 256


@pytest.mark.parametrize("case", [c for c in ALL if c.tie_free], ids=[c.name for c in ALL if c.tie_free])
def test_kept_set_equals_transformers_warpers(case):
    got = ref.kept_set(case.logits.astype(np.float64), **case.params)
    assert np.array_equal(got, _hf_kept(case.logits.astype(np.float64), case.temperature, case.top_k, case.top_p))


@pytest.mark.parametrize("case", sc.PROC_CASES, ids=[c.name for c in sc.PROC_CASES])
def test_processed_rows_are_penalty_ref_rows_and_differ_from_the_raw_kept_set(case):
    mask = np.zeros(case.V, dtype=bool)
    mask[case.seen] = True
    for t in case.ts:
        want = pref.process(case.raw, mask, t=t, repetition_penalty=case.penalty, min_new_tokens=case.min_new, eos_ids=case.eos)
        assert np.array_equal(want.view(np.uint16), case.logits.view(np.uint16))
    raw_keep = ref.kept_set(case.raw.astype(np.float64), **case.params)
    now = sc.draws(case).keep
    assert (raw_keep & ~now).any() and (now & ~raw_keep).any()                  # a sampler that read the raw row keeps another set
    k_raw, k_now = sc.keys_of(case.raw), sc.keys_of(case.logits)
    if case.penalty != 1.0:
        moved = np.flatnonzero((raw_keep != now) & mask)
        assert len(moved) == 1 and abs(int(k_raw[moved[0]] >> 8) - int(k_now[moved[0]] >> 8)) >= 1   # across a high-byte edge
        assert (case.raw[moved[0]] < 0) == (case.penalty < 1.0)                # down by division, up by multiplication
    else:
        assert case.eos and case.raw[list(case.eos)].min() == case.raw.max() and np.isneginf(case.logits[list(case.eos)]).all()
        x = case.raw.astype(np.float32)
        assert ((x - x.max())[np.flatnonzero(now)] < -31).all()                # with the raw maximum every kept mass would be 0


@pytest.mark.parametrize("case", ALL, ids=ids)
def test_checker_accepts_the_restatement_and_refuses_both_mutants(case):
    d = sc.draws(case)
    stats = sc.check_draws(case, d.want)
    assert stats["in_witnesses"] == int(d.in_w.sum()) and stats["worst_gap_over_tol"] == 0.0
    x = case.logits.astype(np.float64)
    # a threshold one value too high: the boundary value is dropped
    fewer = d.keep & (x != d.boundary)
    assert fewer.any()
    with pytest.raises(AssertionError):
        sc.check_draws(case, sc.tokens_of(case, fewer)[0])
    # a threshold one value too low: the first excluded value is kept
    if d.excluded is not None and not case.no_out:
        with pytest.raises(AssertionError):
            sc.check_draws(case, sc.tokens_of(case, d.keep | (x == d.excluded))[0])


def test_checker_refuses_single_wrong_draws():
    case = sc.BY_NAME["k_on_edge_lo00"]
    d = sc.draws(case)
    r = int(np.flatnonzero(d.decisive[0])[0])
    other = int([i for i in case.kept if i != d.want[0, r]][0])
    bad = d.want.copy()
    bad[0, r] = other                                                          # kept, but not the winner of a decisive draw
    with pytest.raises(AssertionError):
        sc.check_draws(case, bad)
    bad = d.want.copy()
    bad[0, 0] = int(np.flatnonzero(~d.keep)[0])                                # not kept
    with pytest.raises(AssertionError):
        sc.check_draws(case, bad)
    with pytest.raises(AssertionError):
        sc.check_draw(case, int(np.flatnonzero(~d.keep)[0]), seed=5, t=2, row=3)
    tok = ref.choose(case.logits, do_sample=True, seed=5, t=2, row=3, **case.params)[0]
    assert sc.check_draw(case, tok, seed=5, t=2, row=3) == 0.0
    assert math.isfinite(sc.check_draws(case, d.want)["worst_gap_over_tol"])
