"""tests/matmul_bound.py's bound is neither wrong nor vacuous: a float32 emulation of each arithmetic class, operation by operation
and in several accumulation orders, stays inside it on every regime at the shapes the GPU tests use, and each injected defect
(a) - (g) exceeds it at some element by at least a factor of 2.  No GPU.

Defect (b), a fold every 256 rows where the kernel says 128, is caught where that fold spans two groups (g = 128: the second group
is folded with the first one's scale and zero point).  Inside one group (g >= 256) it CANNOT exceed the bound by 2: the bound is
linear in the fold blocks' sums, so merging two blocks moves it by one rounding in 44 -- the test records that ratio and asserts
only that it stays below 2 there, so that nobody reads the bound as a check of the fold interval inside a group.

The extended bounds (residual, routing weight, silu pairs, norm prologue) get the same two checks at the end of the file."""
import numpy as np
import pytest

import matmul_bound as mb

ROWS_SHAPES = [(384, 7, 128), (4096, 40, 128), (11008, 24, 128), (1280, 10, 256), (2048, 24, 2048)]
INT_SHAPES = [(512, 40, 128), (4096, 72, 128)]
REF_SHAPES = [(512, 256, 128), (4096, 256, 128)]
ORDERS = ["seq", "rev", "pair"]
F32 = np.float32


def chain(t, order):
    """float32 sum over axis 2 of t [M, F, n, N], one rounding per addition, in the given order"""
    t = t.astype(F32)
    if order == "pair":
        while t.shape[2] > 1:
            if t.shape[2] % 2:
                t = np.concatenate([t, np.zeros_like(t[:, :, :1])], 2)
            t = (t[:, :, 0::2] + t[:, :, 1::2]).astype(F32)
        return t[:, :, 0]
    idx = range(t.shape[2]) if order == "seq" else range(t.shape[2] - 1, -1, -1)
    acc = np.zeros(t.shape[:2] + t.shape[3:], F32)
    for i in idx:
        acc = (acc + t[:, :, i]).astype(F32)
    return acc


def block_sum(t, fold, order):
    """the kernel's shape of a fold block's sum: lanes of 32 contiguous k (eight MFMA steps of four products, taken as 32
    additions in `order`), then the lanes of the block combined in the same order"""
    M, K = t.shape[:2]
    lanes = chain(t.reshape(M, K // 32, 32, -1), order)                  # [M, K/32, N]
    return chain(lanes.reshape(M, K // fold, fold // 32, -1), order)     # [M, F, N]


def defective_operands(case, defect):
    """(x, w, z, s) as the defective kernel would see them: z / s [F128.., N] per GROUP, x [M, K], w [K, N]"""
    x, w, z, s, g = case.x.copy(), case.w.copy(), case.z.copy(), case.s.copy(), case.g
    G = z.shape[0]
    if defect == "c" and G > 1:
        z[1] = case.z[0]
    if defect == "d" and G > 1:
        s[1] = case.s[0]
    if defect == "e":
        x[:, -32:] = 0
    if defect == "f":
        w[8:16] = case.w[0:8]
    return x, w, z, s


def emulate_factorised(case, order, biases=(1024, 64), defect=None, raw=False):
    x, w, z, s = defective_operands(case, defect)
    M, K, N = case.shape
    g = case.g
    fold = 256 if defect == "b" else min(g, mb.FOLD)
    gof = (np.arange(K // fold) * fold) // g                               # the group a fold block takes scale and zero from
    bk = mb._bias_k(K, biases).astype(F32)
    xf = x.astype(F32)
    P = block_sum(xf[:, :, None] * (bk[None, :, None] + w[None].astype(F32)), fold, order)   # exact products
    C0 = block_sum((xf * bk[None])[:, :, None], fold, order)
    SX = block_sum(xf[:, :, None], fold, order)
    if defect == "a":
        with np.errstate(over="ignore"):  # (with the biases 1024 / 64 the partial exceeds the fp16 range: inf is an error too)
            P[:, 0] = P[:, 0].astype(np.float16).astype(F32)
    t = (P - C0).astype(F32)
    t = (t.astype(np.float64) - z[gof][None].astype(np.float64) * SX.astype(np.float64)).astype(F32)   # one fma
    v = (s[gof][None].astype(F32) * t).astype(F32)
    y = chain(v[:, None], order)[:, 0]
    if raw:  # the fp32 sum the epilogue starts from
        return y, K // fold + 2
    return y.astype(np.float16).astype(np.float64), K // fold + 2


def emulate_exact_int(case, order, defect=None):
    x, w, z, s = defective_operands(case, defect)
    M, K, N = case.shape
    g = case.g
    d = w.astype(F32) - np.repeat(z, g, axis=0).astype(F32)
    P = block_sum(x.astype(F32)[:, :, None] * d[None], min(g, mb.FOLD), order)
    gof = (np.arange(P.shape[1]) * min(g, mb.FOLD)) // g
    v = (s[gof][None].astype(F32) * P).astype(F32)
    y = chain(v[:, None], order)[:, 0]
    return y.astype(np.float16).astype(np.float64), P.shape[1] + 2


def emulate_ref_weight(case, order, defect=None):
    x, w, z, s = defective_operands(case, defect)
    c = mb.Case(x, w, z, s, case.g)
    W16 = mb.rounded_weights(c, "gemm")
    if defect == "g":
        W16 = np.where(np.abs(W16.astype(F32)) < 2.0 ** -14, np.float16(0), W16)
    prod = x.astype(F32)[:, :, None] * W16.astype(F32)[None]              # exact: 11 x 11 bits
    y = block_sum(prod, case.x.shape[1], order)[:, 0]
    return y.astype(np.float16).astype(np.float64)


_cases = {}


def case_of(regime, shape, layout, M):
    key = (regime, shape, layout, M)
    if key not in _cases:
        _cases[key] = mb.make_case(regime, *shape, M, layout, seed=1)
    return _cases[key]


def ratio(y, want, bnd):
    err = np.abs(y - want)
    return float(np.where(np.isfinite(err), err / bnd, np.inf).max())


@pytest.mark.parametrize("layout", ["gemm", "gemv", "gemvfast"])
def test_reference_equals_the_oracle_on_the_packed_buffers(oracle, layout):
    for regime in mb.REGIMES:
        c = case_of(regime, (512, 64, 128), layout, 3)
        p = {k: v.numpy() for k, v in mb.pack(c, layout).items()}
        if layout == "gemm":
            want = oracle.linear_gemm_exact(p["x"], p["qweight"], p["qzeros"], p["scales"], c.g)
            W = oracle.dequant_gemm(p["qweight"], p["qzeros"], p["scales"], c.g)
        elif layout == "gemv":
            want = oracle.matmul_exact_gemv(p["x"], p["qweight"], p["qzeros"], p["scales"], c.g)
            W = oracle.dequant_gemv(p["qweight"], p["qzeros"], p["scales"], c.g)
        else:
            want = oracle.matmul_exact_gemvfast(p["x"], p["qweight"], p["scales"], p["qzeros"], c.g)
            W = oracle.dequant_gemvfast(p["qweight"], p["scales"], p["qzeros"], c.g)
        assert np.array_equal(mb.exact(c, layout), want), (layout, regime)
        # the oracle's own dequantiser rounds like rounded_weights (-0 and +0 aside: a zero scale times a negative difference)
        assert np.array_equal(mb.rounded_weights(c, layout).astype(np.float32), W.astype(np.float32)), (layout, regime)


def test_generators_keep_their_promises():
    for regime in mb.REGIMES:
        c = case_of(regime, (4096, 40, 128), "gemv", 4)
        assert c.x.dtype == np.float16 and c.s.dtype == np.float16 and c.w.max() <= 15 and c.z.max() <= 15
        y = mb.exact(c, "gemv")
        a_out = mb._fold_sums(c, "gemv", 128)
        if regime == "biased":
            assert (c.x > 0).all()
        if regime == "outlier":
            assert (np.abs(c.x) == 512).sum(1).tolist() == [1] * 4
        if regime == "flat":
            assert (y[:, 0::4] == 0).all() and (c.w[:, 1::4] == 15).all() and (c.z[:, 2::4] == 15).all()
        if regime == "scales":
            a, b = np.abs(c.s[:-1].astype(np.float64)), np.abs(c.s[1:].astype(np.float64))
            far = (np.maximum(a, b) >= 64 * np.minimum(a, b)) | (np.sign(c.s[:-1]) != np.sign(c.s[1:]))
            assert far.all() and (np.abs(c.s) < 2.0 ** -14).any() and (c.s == 0).any() and (c.s < 0).any() and (c.s == 8).any()
        if regime == "cancel":
            assert (np.abs(y) < 1e-3 * a_out).all()


@pytest.mark.parametrize("shape", ROWS_SHAPES)
def test_factorised_emulation_stays_inside_the_bound(shape):
    for regime in mb.REGIMES:
        c = case_of(regime, shape, "gemv", 2)
        for biases, kernel in (((1024, 64), "gemv_rows"), ((16, 16), "gemv_mfma")):
            for order in ORDERS:
                y, n_out = emulate_factorised(c, order, biases)
                want, bnd = mb.bound(c, "gemv", kernel, n_out=n_out)
                mb.assert_within(y, want, bnd, f"{kernel} emulation {regime} {shape} {order}")


@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integer_emulation_stays_inside_the_bound(shape):
    for regime in mb.REGIMES:
        c = case_of(regime, shape, "gemv", 5)
        for order in ORDERS:
            y, n_out = emulate_exact_int(c, order)
            want, bnd = mb.bound(c, "gemv", "gemv_batch", n_out=n_out, n_p=mb.BATCH_N_P)  # (the depths the GPU test takes from the plan)
            mb.assert_within(y, want, bnd, f"exact-integer emulation {regime} {shape} {order}")


@pytest.mark.parametrize("shape", REF_SHAPES)
def test_reference_weight_emulation_stays_inside_the_bound(shape):
    for regime in mb.REGIMES:
        c = case_of(regime, shape, "gemm", 4)
        want, bnd = mb.bound(c, "gemm", "gemm_tiled")
        for order in ORDERS:
            mb.assert_within(emulate_ref_weight(c, order), want, bnd, f"reference-weight emulation {regime} {shape} {order}")


def caught(emulate, kernel, layout, shapes, M, defect, regimes=mb.REGIMES):
    """the largest error / bound a defect reaches over regimes and shapes (sequential order)"""
    best = 0.0
    for shape in shapes:
        for regime in regimes:
            c = case_of(regime, shape, layout, M)
            out = emulate(c, "seq", defect=defect)
            y, n_out = out if isinstance(out, tuple) else (out, None)
            want, bnd = mb.bound(c, layout, kernel, n_out=n_out)
            best = max(best, ratio(y, want, bnd))
    return best


@pytest.mark.parametrize("defect", ["a", "b", "c", "d", "e", "f"])
def test_factorised_defects_exceed_the_bound(defect):
    shapes = [s for s in ROWS_SHAPES if s[2] == 128 and s[0] % 256 == 0] if defect == "b" else ROWS_SHAPES
    regimes = ("biased", "flat") if defect in "be" else mb.REGIMES
    r = caught(emulate_factorised, "gemv_rows", "gemv", shapes, 2, defect, regimes)
    print(f"factorised defect ({defect}): {r:.3g} x the bound")
    assert r >= 2.0


def test_a_fold_of_256_inside_one_group_is_not_what_the_bound_measures():
    r = caught(emulate_factorised, "gemv_rows", "gemv", [s for s in ROWS_SHAPES if s[2] >= 256], 2, "b", ("biased", "flat"))
    print(f"factorised defect (b) inside one group: {r:.3g} x the bound")
    assert r < 2.0


@pytest.mark.parametrize("defect", ["c", "d", "e", "f"])
def test_exact_integer_defects_exceed_the_bound(defect):
    r = caught(emulate_exact_int, "gemv_batch", "gemv", INT_SHAPES, 5, defect)
    print(f"exact-integer defect ({defect}): {r:.3g} x the bound")
    assert r >= 2.0


@pytest.mark.parametrize("defect", ["c", "d", "e", "f", "g"])
def test_reference_weight_defects_exceed_the_bound(defect):
    r = caught(emulate_ref_weight, "gemm_tiled", "gemm", REF_SHAPES, 4, defect)
    print(f"reference-weight defect ({defect}): {r:.3g} x the bound")
    assert r >= 2.0


# ---- the forms that change the accumulation's input or output (FX_RES, FX_SCALE, FX_PAIRS, FX_NORM), emulated in float32

FX_SHAPE = (4096, 40, 128)


def f16(v):
    return v.astype(np.float16).astype(F32)


def silu_mul_f32(g, u):
    """awq_silu_mul_f32: expf, 1 + e, g / d, q u, each rounded to float32"""
    with np.errstate(over="ignore"):
        e = np.exp(-g.astype(F32)).astype(F32)
    return (((g / (F32(1) + e).astype(F32)).astype(F32)) * u).astype(F32)


def fx_inputs():
    rng = np.random.default_rng(5)
    K, N, _ = FX_SHAPE
    return (4.0 * rng.standard_normal((1, N))).astype(np.float16), (rng.random(K) + 0.5).astype(np.float16)


def normed_f32(x, nw, eps, order, stat_cols=None):
    """the kernel's own activations: float32 sum of squares in `order`, 1 / sqrt in float32, two float32 multiplies, fp16
    (stat_cols: a defect, the statistic taken over the first columns only)"""
    sq = (x.astype(F32) ** 2).astype(F32)[:, :stat_cols]
    ss = chain(sq[:, None, :, None], order)[:, 0, 0]
    inv = (F32(1) / np.sqrt((ss / F32(sq.shape[1])).astype(F32) + F32(eps)).astype(F32)).astype(F32)
    return ((x.astype(F32) * inv[:, None]).astype(F32) * nw.astype(F32)[None]).astype(F32).astype(np.float16)


@pytest.mark.parametrize("order", ORDERS)
def test_fx_form_emulations_stay_inside_the_extended_bounds(order):
    c = case_of("biased", FX_SHAPE, "gemv", 1)
    res, nw = fx_inputs()
    y32, n_out = emulate_factorised(c, order, raw=True)
    # FX_RES: fp16(fp16(sum) + res)
    want, bnd = mb.bound(c, "gemv", "gemv_rows", n_out=n_out, residual=res.astype(np.float64))
    mb.assert_within(f16((f16(y32) + res.astype(F32)).astype(F32)), want, bnd, f"residual {order}")
    # FX_SCALE: fp16(sum * p), p fp32
    for p in (F32(0.3819660113), F32(1.4142135624), F32(-0.75)):
        want, bnd = mb.bound(c, "gemv", "gemv_rows_grouped", n_out=n_out, out_scale=np.array([p]))
        mb.assert_within(f16((y32 * p).astype(F32)), want, bnd, f"routing weight {p} {order}")
    # FX_PAIRS: fp16(silu_mul(fp16(gate), fp16(up)))
    want, bnd = mb.silu_pairs_bound(*mb.bound(c, "gemv", "gemv_rows", n_out=n_out))
    mb.assert_within(f16(silu_mul_f32(f16(y32[:, 0::2]), f16(y32[:, 1::2]))), want, bnd, f"silu pairs {order}")
    # FX_NORM: the kernel's own normalised activations against the reference's, alone and with the two epilogues
    x16, slack = mb.norm_prologue(c.x, nw, 1e-5)
    mine = normed_f32(c.x, nw, 1e-5, order)
    assert (np.abs(mine.astype(np.float64) - x16.astype(np.float64)) <= slack).all()
    assert (slack > 0).mean() < 0.05, "the slack is for values at a rounding boundary only"
    cn = mb.Case(x16, c.w, c.z, c.s, c.g)
    n32, _ = emulate_factorised(mb.Case(mine, c.w, c.z, c.s, c.g), order, raw=True)
    want, bnd = mb.bound(cn, "gemv", "gemv_rows", n_out=n_out, x_slack=slack)
    mb.assert_within(f16(n32), want, bnd, f"norm {order}")
    wr, br = mb.bound(cn, "gemv", "gemv_rows", n_out=n_out, x_slack=slack, residual=res.astype(np.float64))
    mb.assert_within(f16((f16(n32) + res.astype(F32)).astype(F32)), wr, br, f"norm + residual {order}")
    wp, bp = mb.silu_pairs_bound(want, bnd)
    mb.assert_within(f16(silu_mul_f32(f16(n32[:, 0::2]), f16(n32[:, 1::2]))), wp, bp, f"norm + silu pairs {order}")


def test_silu_slope():
    v = np.linspace(-40.0, 40.0, 800001)
    d = np.gradient(mb.silu(v), v)
    assert np.abs(d).max() <= mb.SILU_SLOPE and np.abs(d).max() > 1.09


def test_fx_form_defects_exceed_the_extended_bounds():
    """a residual or routing weight taken from the neighbouring row, gate and up exchanged, a norm weight shifted by one position,
    the norm's statistic taken over half the row: each at least twice the bound somewhere"""
    c = case_of("biased", FX_SHAPE, "gemv", 1)
    res, nw = fx_inputs()
    y32, n_out = emulate_factorised(c, "seq", raw=True)
    found = {}
    want, bnd = mb.bound(c, "gemv", "gemv_rows", n_out=n_out, residual=res.astype(np.float64))
    found["residual of the next column"] = ratio(f16((f16(y32) + np.roll(res, 1, 1).astype(F32)).astype(F32)).astype(np.float64), want, bnd)
    want, bnd = mb.bound(c, "gemv", "gemv_rows_grouped", n_out=n_out, out_scale=np.array([F32(0.3819660113)]))
    found["another pair's routing weight"] = ratio(f16((y32 * F32(0.6180339887)).astype(F32)).astype(np.float64), want, bnd)
    found["routing weight applied after the rounding"] = ratio(f16((f16(y32) * F32(0.3819660113)).astype(F32)).astype(np.float64), want, bnd)
    want, bnd = mb.silu_pairs_bound(*mb.bound(c, "gemv", "gemv_rows", n_out=n_out))
    found["gate and up exchanged"] = ratio(f16(silu_mul_f32(f16(y32[:, 1::2]), f16(y32[:, 0::2]))).astype(np.float64), want, bnd)
    x16, slack = mb.norm_prologue(c.x, nw, 1e-5)
    cn = mb.Case(x16, c.w, c.z, c.s, c.g)
    want, bnd = mb.bound(cn, "gemv", "gemv_rows", n_out=n_out, x_slack=slack)
    for name, mine in (("norm weight shifted by one", normed_f32(c.x, np.roll(nw, 1), 1e-5, "seq")),
                       ("statistic of half the row", normed_f32(c.x, nw, 1e-5, "seq", stat_cols=FX_SHAPE[0] // 2))):
        n32, _ = emulate_factorised(mb.Case(mine.astype(np.float16), c.w, c.z, c.s, c.g), "seq", raw=True)
        found[name] = ratio(f16(n32).astype(np.float64), want, bnd)
    print("FX defects:", {k: round(v, 2) for k, v in found.items()})
    del found["routing weight applied after the rounding"]  # (two roundings where the kernel makes one: up to 1.5 ulp, not 2 x the bound)
    assert min(found.values()) >= 2.0, found
