"""The planner of the batched decode kernel (csrc/gemv_batch.hip plan_batch) through the host-only query awq_gemv_batch_plan: every
M = 1 .. 128 x forced row-part count 0 .. 15 x activation form 0 .. 3 x ring depth 0 .. 3, both layouts, at the 7B / 70B-shard shapes
and ragged ones.  Every accepted plan must be one the kernel can run without touching memory outside its operands -- in particular
no row part may be EMPTY: an empty part's wave groups would name a first row at or past M.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIELDS = ("brs", "rs", "rows_part", "MI", "wk", "passes", "blocks", "tiles_base", "tiles_rem", "lds_bytes", "wt", "RD", "XS",
          "tiles_max", "xs_rows")
GEMV_KERNEL_BATCH = 5
LDS_BUDGET = 160 * 1024
SHAPES = [(4096, 12288), (4096, 4096), (4096, 22016), (11008, 4096),  # the four 7B Linears
          (8192, 1280), (1024, 8192), (8192, 7168), (3584, 8192),     # the four 70B TP = 8 shards
          (2048, 4099), (1024, 200), (256, 16), (16512, 72)]          # ragged N, few tiles, five passes over K


@pytest.fixture(scope="module")
def L():
    from autoawq_amd import _lib

    if not _lib.available():
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def plan(L, M, K, N, form, depth, fast, g=128):
    """dict of the plan, or None where the planner refuses (AWQ_ERR_UNSUPPORTED)"""
    buf = (ctypes.c_int32 * len(FIELDS))()
    rc = L.awq_gemv_batch_plan(M, K, N, g, form, depth, fast, buf)
    assert rc in (0, -3), rc
    return dict(zip(FIELDS, buf)) if rc == 0 else None


def check_plan(p, M, K, N, parts, fast, what):
    brs, rs, rp = p["brs"], p["rs"], p["rows_part"]
    assert (rs * brs - 1) * rp < M, f"{what}: an empty row part ({p})"  # the last part starts below M
    assert rs * brs * rp >= M, f"{what}: rows left without a part ({p})"
    assert 1 <= rp <= 32 and p["MI"] == (2 if rp > 16 else 1), (what, p)
    assert 1 <= brs <= 4 and rs in (1, 2, 4) and (brs == 1 or rs == 1), (what, p)
    if parts >= 2:
        assert rs == 1 and brs <= parts, (what, p)
    elif parts == 1:
        assert brs == 1, (what, p)
    assert p["lds_bytes"] <= LDS_BUDGET, (what, p)
    assert p["wk"] * p["wt"] == 8 and p["wt"] % rs == 0, (what, p)
    # the K range: passes of wk waves x 4 groups x 128 k cover it, and no pass is empty
    span = p["wk"] * 4 * 128
    assert p["passes"] * span >= K and (p["passes"] - 1) * span < K, (what, p)
    # every 16-column tile has exactly one owner: (blocks / brs) blocks of different tiles x (wt / rs) owners each
    assert p["blocks"] >= 1 and p["blocks"] % brs == 0, (what, p)
    if brs > 1:  # whole rounds of the eight XCDs, brs residents of one XCD per tile list (the kernel's block -> (part, owner) map)
        assert p["blocks"] % (8 * brs) == 0, (what, p)
    owners = (p["blocks"] // brs) * (p["wt"] // rs)
    assert p["tiles_base"] * owners + p["tiles_rem"] == (N + 15) // 16, (what, p, owners)
    assert 0 <= p["tiles_rem"] < owners and p["tiles_max"] == p["tiles_base"] + (p["tiles_rem"] > 0), (what, p)
    assert p["xs_rows"] == min(rp, 8), (what, p)
    assert p["RD"] in ((1, 2) if fast else (1, 2, 3)) and p["XS"] in (0, 1), (what, p)
    assert not fast or p["XS"] == 1, (what, p)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("K,N", SHAPES)
def test_every_accepted_plan_is_runnable(L, K, N, fast):
    for M in range(1, 129):
        auto = plan(L, M, K, N, 0, 0, fast)
        for parts in range(16):
            for form in range(4):
                for depth in range(4):
                    what = f"K{K} N{N} M{M} parts{parts} form{form} depth{depth} fast{fast}"
                    p = plan(L, M, K, N, form | (parts << 4), depth, fast)
                    if fast and N % 16:
                        assert p is None, what  # GEMVFast: whole 4-row bundles
                        continue
                    if parts > 4 or (fast and form == 2):
                        assert p is None, what  # at most four row parts; GEMVFast: staged activations only
                        continue
                    if p is None:
                        continue
                    check_plan(p, M, K, N, parts, fast, what)
                    if parts == 0 and form in (0, 3) and depth in (0, 2):
                        assert p == auto, what  # the AUTO plan itself


def test_empty_row_parts_are_never_planned(L):
    """M = 5 in four parts across blocks: two rows a part would start the parts at rows 0, 2, 4 and 6 -- the fourth is empty (its
    wave groups formed x addresses of row 5, past a 5-row tensor).  The planner clamps the part count to the parts the rows fill."""
    for fast in (0, 1):
        p = plan(L, 5, 4096, 11008, 4 << 4, 0, fast)
        assert p is not None and (p["brs"], p["rs"], p["rows_part"]) == (3, 1, 2), p
        p = plan(L, 1, 4096, 11008, 2 << 4, 0, fast)
        assert p is not None and (p["brs"], p["rs"], p["rows_part"]) == (1, 1, 1), p
        for parts in range(5, 16):
            assert plan(L, 100, 4096, 11008, parts << 4, 0, fast) is None, parts
            assert plan(L, 5, 4096, 11008, parts << 4, 0, fast) is None, parts


@pytest.mark.parametrize("fast", [0, 1])
def test_auto_plans_unchanged(L, fast):
    """The AUTO plans at the benched shapes are the ones recorded before the empty-part fix (tests/golden/make_gemv_batch_plans.py)."""
    g = np.load(os.path.join(GOLDEN, "gemv_batch_auto_plans.npz"))
    for s, (K, N) in enumerate(g["shapes"].tolist()):
        for M in range(1, 129):
            p = plan(L, M, K, N, 0, 0, fast)
            want = g["plans"][fast, s, M - 1].tolist()
            got = [p[f] for f in FIELDS] if p is not None else [-1] * len(FIELDS)
            assert got == want, (K, N, M, fast, dict(zip(FIELDS, got)), dict(zip(FIELDS, want)))


@pytest.mark.parametrize("K,N", SHAPES)
def test_auto_never_refuses_what_the_dispatch_sends_it(L, K, N):
    """awq_gemv_auto_kernel (which asks awq_gemv_batch_supports, the AUTO plan) and awq_gemv_forward / awq_gemv_fast_forward's
    chunking (launches of <= 128 rows, fewer where the LDS budget says so, balanced): every launch the dispatch would make on AUTO
    has a plan -- including the smaller chunks the dispatch itself never asks about."""
    for fast in (0, 1):
        for M in list(range(1, 129)) + [129, 200, 255, 257, 300, 513]:
            sup = lambda m: plan(L, min(m, 128), K, N, 0, 0, fast) is not None
            if fast:
                cap = 128
                while cap > 32 and not sup(min(M, cap)):
                    cap //= 2
                if not sup(min(M, cap)) or N % 16:
                    continue
                takes = M >= 5 or 2048 < K <= 4096
            else:
                k = L.awq_gemv_auto_kernel(M, K, N, 128)
                takes = k == GEMV_KERNEL_BATCH
                # awq_gemv_batch_supports is the AUTO plan: the dispatch's condition, restated on the query
                assert takes == ((M >= 5 or (M == 4 and K > 2048) or (M == 3 and K > 6144)) and sup(min(M, 32))), (K, N, M, k)
                if not takes:
                    continue
                cap = 128
                while cap > 32 and not sup(min(M, cap)):
                    cap //= 2
            if not takes:
                continue
            nchunk = (M + cap - 1) // cap
            rows = (M + nchunk - 1) // nchunk
            for m0 in range(0, M, rows):
                mm = min(rows, M - m0)
                p = plan(L, mm, K, N, 0, 0, fast)
                assert p is not None, (K, N, M, mm, fast)
                check_plan(p, mm, K, N, 0, fast, f"K{K} N{N} M{M} chunk {mm} fast{fast}")


def test_plan_query_refuses_bad_arguments(L):
    buf = (ctypes.c_int32 * len(FIELDS))()
    assert L.awq_gemv_batch_plan(8, 4096, 4096, 128, 0, 0, 0, None) == -6
    for M, K, N, g in [(0, 4096, 4096, 128), (129, 4096, 4096, 128), (8, 4096, 4096, 64), (8, 4100, 4096, 128), (8, 4096, 0, 128)]:
        assert L.awq_gemv_batch_plan(M, K, N, g, 0, 0, 0, buf) == -3, (M, K, N, g)
