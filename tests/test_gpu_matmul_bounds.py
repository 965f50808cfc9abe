"""Every int4 matmul kernel on adversarial data, element by element against the bound derived from its own arithmetic
(tests/matmul_bound.py): activations of one sign, an outlier channel that meets w == z, whole columns of w == z, subnormal / zero /
negative / large scales that change by 2^6 from group to group, and groups that cancel.  Each kernel is forced by its flag and
`ops.last_kernel()` is asserted; a shape a kernel refuses raises (an error, not a skip).  The forms of awq_gemv_forward_ex (residual,
silu pairs, norm prologue) and the grouped MoE launches (routing weights) are held to the bound extended by their roundings.  The one-hot sweeps at the end read every
k position of a row once: y == W^T[k] bit for bit against the dequantise kernel.

MATMUL_BOUND_RECORD=<file>: every case appends "kernel layout K N g M variant regime err/bound ulps" (recorded, not asserted)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import matmul_bound as mb

pytestmark = pytest.mark.gpu

TILE16, ROWS, LDS, PREFILL, BATCH = 1, 2, 3, 4, 5          # AWQ_GEMV_KERNEL_*
VALU, MFMA_GEMV, TILED, REGB, SKINNY = 2, 3, 4, 5, 6       # AWQ_GEMM_KERNEL_*


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()
    return _ops


_cache, _bounds = {}, {}


def operands(regime, K, N, g, M, layout):
    """(case, device buffers) of the largest M a shape is used with, made once; rows are sliced from it"""
    key = (regime, K, N, g, M, layout)
    if key not in _cache:
        case = mb.make_case(regime, K, N, g, M, layout, seed=7)
        _cache[key] = (case, {k: v.cuda() for k, v in mb.pack(case, layout).items()})
    return _cache[key]


def record(kernel, layout, shape, M, variant, regime, y, want, bnd):
    r, ulps = mb.worst(y, want, bnd)
    line = f"{kernel} {layout} K{shape[0]} N{shape[1]} g{shape[2]} M{M} {variant or 'default'} {regime} {r:.4f} {ulps:.3f}"
    print(line)
    path = os.environ.get("MATMUL_BOUND_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def run_regimes(ops, kernel, layout, shape, Ms, call, variant="", bound_kernel=None, regimes=mb.REGIMES, top=None, depths=None):
    K, N, g = shape
    top = top or max(Ms)  # (the rows the shape's case is made with)
    for regime in regimes:
        case, d = operands(regime, K, N, g, top, layout)
        for M in Ms:
            y = call(d, M).cpu().numpy().astype(np.float64)
            assert ops.last_kernel() == kernel, (ops.last_kernel(), kernel)
            known = depths(M) if depths else {}  # (n_p / n_out of this launch where its plan reports the geometry)
            bkey = (regime, shape, top, M, layout, bound_kernel or kernel, tuple(sorted(known.items())))  # (a case is made for its largest M)
            if bkey not in _bounds:
                _bounds[bkey] = mb.bound(case.rows(M), layout, bound_kernel or kernel, **known)
            want, bnd = _bounds[bkey]
            record(kernel, layout, shape, M, variant, regime, y, want, bnd)
            mb.assert_within(y, want, bnd, f"{kernel} {variant} {regime} K{K} N{N} g{g} M{M}")


def gemv_call(ops, g, **flags):
    return lambda d, M: ops.gemv_forward(d["x"][:M], d["qweight"], d["scales"], d["qzeros"], g, flags=ops.gemm_flags(**flags))


def gemm_call(ops, **flags):
    return lambda d, M: ops.gemm_forward(d["x"][:M], d["qweight"], d["scales"], d["qzeros"], None, flags=ops.gemm_flags(**flags))


def fast_call(ops, g, **flags):
    return lambda d, M: ops.gemv_fast_forward(d["x"][:M], d["qweight"], d["scales"], d["qzeros"], g, flags=ops.gemm_flags(**flags))


# ------------------------------------------------------------------ GEMV layout

ROWS_SHAPES = [(384, 7, 128), (4096, 40, 128), (11008, 24, 128), (1280, 10, 256), (2048, 24, 2048)]


# The launcher's own slot count depends on M (pick_sl, gemv_rows.hip:746: the smallest of 1, 2, 3, 4, 6, 8 that covers the row's
# ceil(K / 2048) slots, capped at 8 / 3 / 1 slots for M = 1 / 2 / 4): 1, 2, 6, 1, 1 slots at M = 1 on the five shapes, 1, 2, 3, 1, 1
# at M = 2 and 1 everywhere at M = 4.  The forced count differs from it at EVERY M: 2 where the default is 1 (16 SL M <= 128
# registers allow 2 slots at M = 4, :808), and at K = 4096 one slot at M = 1 and 2, two at M = 4; at K = 11008 two slots against 6, 3, 1.
ROWS_DEFAULT_SLOTS = {384: (1, 1, 1), 4096: (2, 2, 1), 11008: (6, 3, 1), 1280: (1, 1, 1), 2048: (1, 1, 1)}  # at M = 1, 2, 4


@pytest.mark.parametrize("slots", [0, "forced"])
@pytest.mark.parametrize("shape", ROWS_SHAPES)
def test_gemv_rows(ops, shape, slots):
    def run(Ms, nlog):
        run_regimes(ops, "gemv_rows", "gemv", shape, Ms, gemv_call(ops, shape[2], kernel=ROWS, nlog=nlog), f"slots{nlog}", top=4)

    if slots == 0:
        run([1, 2, 4], 0)
        return
    forced = {1: 1, 2: 1, 4: 2} if shape[0] == 4096 else {1: 2, 2: 2, 4: 2}
    for i, M in enumerate((1, 2, 4)):
        assert forced[M] != ROWS_DEFAULT_SLOTS[shape[0]][i]
    for nlog in sorted(set(forced.values())):
        run([M for M in (1, 2, 4) if forced[M] == nlog], nlog)


# ---- the FX forms of awq_gemv_forward_ex (batch 1): residual, silu pairs and the norm prologue on `biased` at (4096, 40, 128),
# each against the plain bound extended by the roundings the form adds (tests/matmul_bound.py, "the FX forms")
FX_SHAPE = (4096, 40, 128)


@pytest.mark.parametrize("form", ["res", "pairs", "norm", "norm_res", "norm_pairs"])
def test_gemv_rows_fx_forms(ops, form):
    K, N, g = FX_SHAPE
    case4, d = operands("biased", K, N, g, 4, "gemv")
    case = case4.rows(1)
    rng = np.random.default_rng(5)
    res = (4.0 * rng.standard_normal((1, N))).astype(np.float16)
    nw = (rng.random(K) + 0.5).astype(np.float16)
    eps = 1e-5
    kw, slack = {}, None
    if "norm" in form:
        x16, slack = mb.norm_prologue(case.x, nw, eps)
        case = mb.Case(x16, case.w, case.z, case.s, g, "biased")
        kw.update(norm_weight=torch.from_numpy(nw).cuda(), norm_eps=eps)
    if "res" in form:
        kw.update(add_residual=torch.from_numpy(res).cuda())
    if "pairs" in form:
        kw.update(silu_pairs=True)
    y = ops.gemv_forward_ex(d["x"][:1], d["qweight"], d["scales"], d["qzeros"], g, **kw).cpu().numpy().astype(np.float64)
    assert ops.last_kernel() == "gemv_rows"
    want, bnd = mb.bound(case, "gemv", "gemv_rows", x_slack=slack, residual=res.astype(np.float64) if "res" in form else None)
    if "pairs" in form:
        want, bnd = mb.silu_pairs_bound(want, bnd)
    assert y.shape == want.shape
    record("gemv_rows", "gemv", FX_SHAPE, 1, f"fx_{form}", "biased", y, want, bnd)
    mb.assert_within(y, want, bnd, f"gemv_rows fx {form} biased K{K} N{N} g{g}")


def batch_depths(shape, parts):
    """n_p and n_out of gemv_batch from awq_gemv_batch_plan's wk and passes (fields 4 and 5), the largest over the plans of
    every row count up to M (the wrapper may hand the library the rows in chunks)"""
    from autoawq_amd import _lib

    K, N, g = shape

    def depths(M):
        buf = (ctypes.c_int32 * 15)()
        n_out = 0
        for m in range(1, M + 1):
            if _lib.lib().awq_gemv_batch_plan(m, K, N, g, parts << 4, 0, 0, buf) == 0:
                n_out = max(n_out, mb.batch_n_out(buf[4], buf[5]))
        assert n_out, "the planner refuses the shape"
        return {"n_p": mb.BATCH_N_P, "n_out": n_out}
    return depths


# waves = 4 at 33 rows: parts of 9, 8, 8, 8 rows; waves = 2 at 17: 9 and 8 -- a ragged last part either way
@pytest.mark.parametrize("waves", [0, "forced"])
@pytest.mark.parametrize("shape", [(512, 40, 128), (4096, 72, 128)])
def test_gemv_batch(ops, shape, waves):
    if waves == 0:
        run_regimes(ops, "gemv_batch", "gemv", shape, [5, 17, 33], gemv_call(ops, shape[2], kernel=BATCH), depths=batch_depths(shape, 0))
    else:
        run_regimes(ops, "gemv_batch", "gemv", shape, [33], gemv_call(ops, shape[2], kernel=BATCH, waves=4), "parts4", depths=batch_depths(shape, 4))
        run_regimes(ops, "gemv_batch", "gemv", shape, [17], gemv_call(ops, shape[2], kernel=BATCH, waves=2), "parts2", depths=batch_depths(shape, 2))


@pytest.mark.parametrize("shape", [(512, 40, 32), (1024, 72, 64), (4096, 40, 128)])
def test_gemv_nk(ops, shape):
    run_regimes(ops, "gemv_nk", "gemv", shape, [1, 3, 16], gemv_call(ops, shape[2], kernel=TILE16))


# gemv_lds takes group sizes that are multiples of 128 only, 2 <= M and M K <= 32768 (awq_gemv_lds_supports): the issue's
# (512, 40, 32) and (1024, 72, 64) become g = 128, and the rows 2, 3 and 8
@pytest.mark.parametrize("shape", [(512, 40, 128), (1024, 72, 128), (4096, 40, 128)])
def test_gemv_lds(ops, shape):
    run_regimes(ops, "gemv_lds", "gemv", shape, [2, 3, 8], gemv_call(ops, shape[2], kernel=LDS))


@pytest.mark.parametrize("shape", [(512, 40, 128), (4096, 40, 128)])
def test_gemm_regb_on_the_gemv_layout(ops, shape):
    run_regimes(ops, "gemm_regb_nk", "gemv", shape, [40], gemv_call(ops, shape[2], kernel=PREFILL))


# ------------------------------------------------------------------ GEMM layout

MFMA_VARIANTS = {"default": {}, "splitk2": {"splitk": 2}, "two_pass": {"splitk": 2, "two_pass": True}, "wpl2": {"nlog": 2}, "wpl4": {"nlog": 4}}


@pytest.mark.parametrize("variant", list(MFMA_VARIANTS))
@pytest.mark.parametrize("shape", [(512, 256, 128), (4096, 256, 128), (1024, 256, 64)])
def test_gemv_mfma(ops, shape, variant):
    Ms = [1, 8] if variant == "wpl4" else [1, 8, 9, 16]  # four words per lane serve at most 8 rows (awq_gemv_mfma_supports)
    run_regimes(ops, "gemv_mfma", "gemm", shape, Ms, gemm_call(ops, kernel=MFMA_GEMV, **MFMA_VARIANTS[variant]), variant)


@pytest.mark.parametrize("kernel,code,Ms,splitk", [("gemm_skinny", SKINNY, [17, 64], 0), ("gemm_skinny", SKINNY, [17, 64], 2),
                                                   ("gemm_tiled", TILED, [65, 130], 0), ("gemm_tiled", TILED, [65, 130], 2),
                                                   ("gemm_regb", REGB, [128, 300], 0), ("gemv_valu", VALU, [1, 4], 0),
                                                   ("gemv_valu", VALU, [1, 4], 2)])
@pytest.mark.parametrize("shape", [(512, 256, 128), (4096, 256, 128)])
def test_reference_weight_kernels(ops, shape, kernel, code, Ms, splitk):
    run_regimes(ops, kernel, "gemm", shape, Ms, gemm_call(ops, kernel=code, splitk=splitk), f"splitk{splitk}")


# gemm_regb has no split-K form (autoawq_amd/csrc/gemm_regb.hip takes no such flag), hence its one variant above


# ------------------------------------------------------------------ grouped (MoE decode): E = 2, three pairs, expert 0 twice

GROUPED_IDS = (0, 1, 0)
ROUTING = np.array([0.6180339887, 0.3819660113, 1.4142135624], np.float32)   # fp32 routing weights, one per pair
_grouped = {}


def grouped_operands(regime, shape, layout):
    """two experts' weights (seeds apart), three activation rows; pair t = row t on expert GROUPED_IDS[t]"""
    key = (regime, shape, layout)
    if key not in _grouped:
        K, N, g = shape
        experts = [mb.make_case(regime, K, N, g, 3, layout, seed=11 + e) for e in range(2)]
        x = experts[0].x
        pairs = [mb.Case(x[t:t + 1], experts[e].w, experts[e].z, experts[e].s, g, regime) for t, e in enumerate(GROUPED_IDS)]
        for c in pairs:
            y = mb.exact(c, layout)
            assert np.isfinite(y).all() and np.abs(y).max() * float(ROUTING.max()) < 60000.0
        packed = [mb.pack(c, layout) for c in experts]
        d = {k: torch.stack([p[k] for p in packed]).cuda() for k in ("qweight", "scales", "qzeros")}
        d["x"] = torch.from_numpy(x).cuda()
        d["ids"] = torch.tensor(GROUPED_IDS, dtype=torch.int32).view(3, 1).cuda()
        d["w"] = torch.from_numpy(ROUTING).view(3, 1).cuda()
        _grouped[key] = (pairs, d)
    return _grouped[key]


def check_grouped(ops, kernel, layout, shape, regime, variant, weighted, forward):
    pairs, d = grouped_operands(regime, shape, layout)
    y = forward(d).cpu().numpy().astype(np.float64)
    assert ops.last_kernel() == kernel and y.shape == (3, 1, shape[1])
    for t, c in enumerate(pairs):
        want, bnd = mb.bound(c, layout, kernel, out_scale=ROUTING[t:t + 1] if weighted else None)
        record(kernel, layout, shape, 1, f"{variant}_pair{t}", regime, y[t], want, bnd)
        mb.assert_within(y[t], want, bnd, f"{kernel} {variant} {regime} pair {t} (expert {GROUPED_IDS[t]})")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("regime", ["biased", "scales"])
def test_gemv_rows_grouped(ops, regime, weighted):
    shape = (512, 40, 128)
    check_grouped(ops, "gemv_rows_grouped", "gemv", shape, regime, "routed" if weighted else "plain", weighted,
                  lambda d: ops.grouped_gemv_forward(d["x"], d["qweight"], d["scales"], d["qzeros"], d["ids"], shape[2],
                                                     topk_weights=d["w"] if weighted else None))


# block_rows 16: the reference's token blocks; 8: the selector-row form of decode-sized batches
@pytest.mark.parametrize("block_rows", [16, 8])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("regime", ["biased", "scales"])
def test_gemv_mfma_grouped(ops, regime, weighted, block_rows):
    shape = (512, 256, 128)

    def forward(d):
        sorted_ids, expert_ids, post_pad = ops.moe_align_block_size(d["ids"], block_rows, 2)
        return ops.grouped_gemm_forward(d["x"].view(3, 1, -1), d["qweight"], d["scales"], d["qzeros"], d["w"], sorted_ids, expert_ids,
                                        post_pad, weighted, block_rows=block_rows)

    check_grouped(ops, "gemv_mfma_grouped", "gemm", shape, regime, f"rows{block_rows}_" + ("routed" if weighted else "plain"), weighted, forward)


# ------------------------------------------------------------------ GEMVFast layout

@pytest.mark.parametrize("shape", [(512, 64, 128), (4096, 128, 128)])
def test_gemvfast_kernels(ops, shape):
    g = shape[2]
    run_regimes(ops, "gemv_fast", "gemvfast", shape, [1, 8, 40], fast_call(ops, g, kernel=1))
    run_regimes(ops, "gemv_batch_fast", "gemvfast", shape, [1, 8, 40, 300], fast_call(ops, g, kernel=BATCH))
    prefill = lambda d, M: ops.gemv_fast_prefill(d["x"][:M], d["qweight"], d["scales"], d["qzeros"], g)  # noqa: E731
    run_regimes(ops, "repack_fast+gemm_regb_fz", "gemvfast", shape, [40, 300], prefill, bound_kernel="gemm_regb_fz")


# ------------------------------------------------------------------ every k is read once, by the right lane

def one_hot_sweep(K, rows, forward, Wt):
    """one-hot activations over all k, `rows` per launch: row i of launch j is e_(j rows + i); y must equal W^T[:, k] bit for bit"""
    eye = torch.eye(rows, dtype=torch.float16, device="cuda")
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    bad_at = torch.full((), K, dtype=torch.int64, device="cuda")
    for k0 in range(0, K, rows):
        x = torch.zeros((rows, K), dtype=torch.float16, device="cuda")
        x[:, k0:k0 + rows] = eye
        y = forward(x)
        same = (y == Wt[:, k0:k0 + rows].t()).all()
        bad_at = torch.where(ok & ~same, torch.full_like(bad_at, k0), bad_at)
        ok = ok & same
    assert bool(ok), f"one-hot rows {int(bad_at)} .. {int(bad_at) + rows - 1} of K = {K} differ from the dequantised weight"


@pytest.mark.parametrize("shape", [(384, 7, 128), (4096, 40, 128), (11008, 24, 128)])
def test_gemv_rows_reads_every_k_once(ops, shape):
    K, N, g = shape
    _, d = operands("scales", K, N, g, 4, "gemv")
    Wt = ops.dequantize_weights_gemv(d["qweight"], d["scales"], d["qzeros"], g)
    one_hot_sweep(K, 4, lambda x: ops.gemv_forward(x, d["qweight"], d["scales"], d["qzeros"], g, flags=ops.gemm_flags(kernel=ROWS)), Wt)
    assert ops.last_kernel() == "gemv_rows"


def test_gemv_batch_reads_every_k_once(ops):
    K, N, g = 512, 40, 128
    _, d = operands("scales", K, N, g, 33, "gemv")
    Wt = ops.dequantize_weights_gemv(d["qweight"], d["scales"], d["qzeros"], g)
    one_hot_sweep(K, 32, lambda x: ops.gemv_forward(x, d["qweight"], d["scales"], d["qzeros"], g, flags=ops.gemm_flags(kernel=BATCH)), Wt)
    assert ops.last_kernel() == "gemv_batch"


def test_gemv_mfma_reads_every_k_once(ops):
    K, N, g = 512, 256, 128
    _, d = operands("scales", K, N, g, 16, "gemm")
    Wt = ops.dequantize_weights(d["qweight"], d["scales"], d["qzeros"]).t().contiguous()
    one_hot_sweep(K, 16, lambda x: ops.gemm_forward(x, d["qweight"], d["scales"], d["qzeros"], None, flags=ops.gemm_flags(kernel=MFMA_GEMV)), Wt)
    assert ops.last_kernel() == "gemv_mfma"


def test_gemv_fast_reads_every_k_once(ops):
    K, N, g = 512, 64, 128
    _, d = operands("scales", K, N, g, 300, "gemvfast")
    Wt = ops.dequantize_weights_gemv_fast(d["qweight"], d["scales"], d["qzeros"], g)
    one_hot_sweep(K, 16, lambda x: ops.gemv_fast_forward(x, d["qweight"], d["scales"], d["qzeros"], g, flags=ops.gemm_flags(kernel=1)), Wt)
    assert ops.last_kernel() == "gemv_fast"
