"""float64 reference, adversarial inputs and a per-element error bound derived from the int4 matmul kernels' arithmetic, for the tests.

A `Case` holds the LOGICAL operands -- x [M, K] fp16, nibbles w [K, N], zero points z [G, N], scales s [G, N] fp16, group size g --
and `pack(case, layout)` lays them out as the GEMM, GEMV or GEMVFast buffers the kernels read (autoawq_amd/utils/packing.py).
`exact(case, layout)` is the exact product in float64 (equal to oracle.linear_gemm_exact / matmul_exact_gemv / matmul_exact_gemvfast
on the packed buffers, tests/test_matmul_bound_cpu.py checks that), `rounded_weights` the reference's fp16 weight fp16((w - z) s)
(GEMVFast: fp16(w s + qzeros)), one IEEE rounding with subnormals kept.  `bound(case, layout, kernel, ...)` returns (want, bound),
`assert_within` compares a kernel's output with both.

Notation: u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u), ulp16(y) = max(|y|, 2^-14) 2^-10.  A FOLD BLOCK f is the run of
k positions whose products are accumulated before scale and zero point are applied: min(g, 128) positions in every kernel below
(a group, and at least every 128 rows).  d_f = sum_{k in f} x_k (w_k - z_f), exact.  Every product x_k (bias + w_k) of an fp16
value and an integer below 2048 is exact in fp32, so only the ADDITIONS round.  A chain of n fp32 additions in any order is off by
at most gamma(n) sum |terms|.  An MFMA step's internal order is not specified: a step over k products counts as k + 1 sequential
roundings (as tests/attn_bound.py does).  1.01 covers the second-order products of the first-order terms (all below 1e-2).

Factorised class:  y = sum_f s_f (P_f - C_f),  P_f = sum x_k (bias_k + w_k),  C_f = sum x_k (bias_k + z_f)  (as C0 + z SX or in one sum)
-----------------------------------------------------------------------------------------------------------------------------------
    |y~ - y| <= ulp16(y) + 1.01 [ sum_f |s_f| ( gamma(n_P) sum_{k in f} |x_k| (bias_k + w_k) + gamma(n_C) sum_{k in f} |x_k| (bias_k + z_f) )
                                  + gamma(n_out) sum_f |s_f d_f| ]
(the issue's formula with the sums over groups taken over fold blocks: that is what the kernels add up when g > 128).
n_P / n_C: the roundings between the first product and the folded value, INCLUDING the fold's own subtraction and fma;
n_out: the scale multiply and every addition of folded values down to the fp32 value that is rounded to fp16.

  gemv_rows (autoawq_amd/csrc/gemv_rows.hip; biases 1024 on even k, 64 on odd k: awq_mfma_decode.h pairb, gemv_rows.hip:490-493, :562-563)
    * P: a lane's 32 products by eight v_mfma_f32_4x4x4_16b_f16 steps of 4 (:560-569): 8 x 5 = 40; `pa + pb` with pb = 0 is exact
      (:588); the 4 x 4 transpose-reduce of the quad adds 2 (:607-609); `rq - c0` and the fma round once each (:610): n_P = 44.
    * C0 / SX: the same eight MFMA steps against constant rows (:496-497), two DPP additions (:500-503), then the same subtraction
      and fma: n_C = 44.  A quad is 128 k and never straddles a group (awq_gemv_rows_supports, :767): the fold is every 128 k for
      every g, its scale and zero point the group's.
    * out: scl * (...) (:610), two row rotations (:611-612), (v0 + v1) + (v2 + v3) and the running sum over the wk * SL slots
      (:656, :690): n_out = 5 + wk SL.  The launch reports no geometry; the worst case over the slot counts it can choose
      (SL in 1, 2, 3, 4, 6, 8 and wk = ceil(slots / SL), pick_sl :746) is wk SL <= slots + 7, slots = ceil(K / 2048).
    * the FX forms (the roundings they add to the plain bound b of want = W x):
      FX_RES stores fp16(fp16(W x) + res) (:668): h = fp16(sum) is within b of want, h + res is formed in fp32 and rounded to
        fp16, at most half an ulp at |h + res| <= |want + res| + b:   b + ulp16(want + res) + 2^-10 b.
      FX_SCALE (grouped form) multiplies the fp32 sum by the fp32 routing weight p before the one rounding (:673); gemv_mfma's
        grouped form does the same (gemv_mfma.hip:473).  One more fp32 rounding, u |want|, and everything scales by |p|:
        ulp16(p want) + 1.01 |p| (terms + u |want|).
      FX_PAIRS stores fp16(silu_mul(fp16(G~), fp16(U~))) for the row pair (gate, up) (:662-663); the reference is
        silu(G) U in float64 of the exact products G, U with plain bounds b_G, b_U (their ulp16 terms are the two fp16
        roundings).  |silu'| <= 1.1 everywhere (its maximum is 1.0998 at x = 2.3994), so
        E1 = (|silu(G)| + 1.1 b_G) b_U + 1.1 |U| b_G bounds the exact function of the rounded pair; awq_silu_mul_f32
        (awq_device.h:51-59: expf, 1 + e, g / d, q u; the HIP math API states 1 ulp for expf and 2.5 ulp for the division where
        it is not correctly rounded: 2 + 1 + 5 + 1 = 9 u, taken as gamma(16)) gives E2 = E1 + gamma(16) (|want| + E1), and the
        last rounding half an ulp at |want| + E2:   ulp16(want) + (1 + 2^-10) E2.
      FX_NORM replaces x by fp16(fp32(fp32(x) inv) fp32(w)), inv = rsqrtf(ss / K + eps) (:115-128, :426, :473).  ss adds K exact
        squares, all positive: per lane four v_dot2 chains of 4 (two roundings each: 8), 4 SL <= 24 additions of them (:416-424,
        :463-472; SL <= 6 with the norm, :721), wave_sum's 4 + 2 (:404-411): relative error gamma(38); / K and + eps: gamma(40)
        on the argument, half of it on inv; rsqrtf: the HIP math API states 1 ulp, counted as 2 (4 u); the two multiplies 2 u:
        20 + 4 + 2 = 26 u, taken as e = 1.01 gamma(32).  The last rounding is monotone, so the kernel's activation lies between
        fp16(|xn| (1 - e)) and fp16(|xn| (1 + e)), xn the exact normalised value.  The reference takes x16 = fp16(xn) (one
        rounding of the exact value) as ITS activations; slack_k = the larger distance from |x16_k| to those two ends (0 unless
        xn_k lies within e of a rounding boundary).  The plain bound is then taken at |x| + slack, with
        D = sum_k slack_k |W_k| added to sum_f |s_f d_f| and (1 + 2^-10) D to the bound (the moved product and its ulp).
        gemv_mfma's NORM staging (awq_gemm_forward_normed / _ex, gemv_mfma.hip:254-308) takes the same extension with its own e:
        norm_prologue(..., depth) with the depths tests/norm_rope_bound.py counts (its statistic pass, or the producer's ssq_out).
  gemv_nk (autoawq_amd/csrc/gemv_nk.hip; biases 1024 / 64, :62-68), gemv_lds (autoawq_amd/csrc/gemv_lds.hip; 1024 / 64, :144-147),
  gemv_mfma (autoawq_amd/csrc/gemv_mfma.hip; bias 16, :15-16, :104), gemv_fast (autoawq_amd/csrc/gemv_fast.hip; bias 16, :59) and the GEMVFast form of
  gemv_batch (autoawq_amd/csrc/gemv_batch.hip:143, :447-448; bias 16)
    * P and C by v_mfma_f32_16x16x32_f16 steps (gemv_nk.hip:167-183: four steps per 128 k into `acc` and into `accz`), or for
      gemv_lds's C0 / SX by v_dot2 chains (gemv_lds.hip:162-178).  Their exact depth depends on template parameters the launch does
      not report, so these kernels take the WORST CASE of any order: every one of the <= 128 products of a fold block added
      sequentially, one more rounding per MFMA step, and 16 for cross-lane additions, the (bias + z) sx product, the subtraction
      and the fma: n_P = n_C = 128 + 4 + 16 = 148.
    * out: one fma per fold (gemv_nk.hip:188), then the waves of the block, the in-launch split-K slices or the second pass's
      slabs (gemv_mfma.hip:433, :660).  Worst case, every fold of the row in one chain plus 64 for waves (<= 16), slices (<= 32)
      and the epilogue: n_out = K / fold + 64.
    * GEMVFast stores qzeros = fp16(-(s z)) and folds s (P - 16 sx) + qzeros sx (gemv_fast.hip:168): the C term's weight
      |s_f| (bias + z_f) becomes 16 |s_f| + |qzeros_f|, and d_f = sum x_k (w_k s_f + qzeros_f) carries the scale already.

Exact-integer class: gemv_batch on the GEMV layout (autoawq_amd/csrc/gemv_batch.hip:33: four packed subtracts of (bias + z), w - z exact in fp16)
-----------------------------------------------------------------------------------------------------------------------------------
    |y~ - y| <= ulp16(y) + 1.01 [ gamma(n_P) sum_f |s_f| sum_{k in f} |x_k (w_k - z_f)| + gamma(n_out) sum_f |s_f d_f| ]
(group size 128 only: awq_gemv_batch_plan refuses the others).  Here the launch's geometry is known from awq_gemv_batch_plan:
    * P: a group's 128 products by four v_mfma_f32_16x16x32_f16 steps into a zeroed gacc (gemv_batch.hip:482-498): n_P = 4 x 33 = 132.
    * out: one fma per group, acc = fma(s, gacc, acc), over the GW = 4 groups a wave owns in a pass (:499-502, acc zeroed per pass
      and tile :404); the wk waves' partial tiles are added (wk - 1, :527-528) and the passes' sums (passes - 1, :530, :537):
      n_out = 4 + (wk - 1) + (passes - 1), wk and passes as the plan reports them.  The Python wrapper may hand the rows to the
      library in chunks; the tests take the largest n_out over the plans of every row count up to M.
The GEMVFast form of the kernel (gemv_batch_fast), the other factorised kernels and the reference-weight class keep their worst
case of any order: the other plan functions (awq_gemv_auto_kernel, awq_gemm_auto_kernel) name the kernel that runs, not its
waves, slices or tiles, and no launch reports them.

Reference-weight class: gemm_tiled, gemm_regb (and its FZ / NK forms), gemm_skinny, gemv_valu
-----------------------------------------------------------------------------------------------------------------------------------
These multiply x by the reference's own fp16 weight W16 and accumulate in fp32 over the whole of K, so the reference is the float64
product of W16 and weight rounding is NOT part of the error: a weight that differs from IEEE fp16((w - z) s) in one bit fails.
    |y~ - x W16| <= ulp16(y) + 1.01 gamma(n_acc) sum_k |x_k W16_k|,     n_acc = K + K / 32 + 64
(worst case of any order: K products one after the other, one rounding per 32-wide MFMA step, 64 for waves, split-K and epilogue).
"""
from dataclasses import dataclass

import numpy as np
import torch

U = 2.0 ** -24
FOLD = 128          # "at least every 128 rows": gemv_mfma.hip:24-25, gemv_nk.hip:24-25, gemv_lds.hip:21, gemv_fast.hip:17, gemv_rows.hip:767
ROWS_N_P = ROWS_N_C = 44
WORST_N_FOLD = FOLD + FOLD // 32 + 16

FACTORISED = {  # kernel -> (bias on even k, bias on odd k)
    "gemv_rows": (1024, 64), "gemv_rows_grouped": (1024, 64), "gemv_nk": (1024, 64), "gemv_lds": (1024, 64),
    "gemv_mfma": (16, 16), "gemv_mfma_grouped": (16, 16), "gemv_fast": (16, 16), "gemv_batch_fast": (16, 16),
}
EXACT_INT = ("gemv_batch",)
REF_WEIGHT = ("gemm_tiled", "gemm_regb", "gemm_regb_nk", "gemm_regb_fz", "gemm_skinny", "gemv_valu")
REGIMES = ("biased", "outlier", "flat", "scales", "cancel")


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp16(y):
    return np.maximum(np.abs(y), 2.0 ** -14) * 2.0 ** -10


@dataclass
class Case:
    x: np.ndarray   # [M, K] float16
    w: np.ndarray   # [K, N] uint8, 0..15
    z: np.ndarray   # [G, N] uint8, 0..15
    s: np.ndarray   # [G, N] float16
    g: int
    regime: str = ""

    @property
    def shape(self):
        return self.x.shape[0], self.x.shape[1], self.w.shape[1]

    def rows(self, M):
        return Case(self.x[:M], self.w, self.z, self.s, self.g, self.regime)


# ------------------------------------------------------------------ the three layouts

def pack(case, layout):
    """the kernels' buffers (torch, host): gemm -> qweight [K, N/8], qzeros [G, N/8], scales [G, N]; gemv -> qweight [N, K/8],
    qzeros [N, ZW], scales [N, 8 ZW]; gemvfast -> qweight int16 [N/4, K], scales / qzeros fp16 [8 ZW, N], qzeros = fp16(-(s z))"""
    from autoawq_amd.utils.packing import (GEMV_ORDER, calculate_zeros_width, pack_intweight_fast, pack_rows_int4, pack_zeros_nk)

    M, K, N = case.shape
    G = K // case.g
    w, z, s = torch.from_numpy(case.w.astype(np.int32)), torch.from_numpy(case.z.astype(np.int32)), torch.from_numpy(case.s)
    x = torch.from_numpy(case.x)
    if layout == "gemm":
        return {"x": x, "qweight": pack_rows_int4(w), "qzeros": pack_rows_int4(z), "scales": s.contiguous()}
    zw = calculate_zeros_width(K, case.g)
    if layout == "gemv":
        sc = torch.zeros((N, 8 * zw), dtype=torch.float16)
        sc[:, :G] = s.t()
        return {"x": x, "qweight": pack_rows_int4(w.t().contiguous(), GEMV_ORDER), "qzeros": pack_zeros_nk(z.t().contiguous(), zw), "scales": sc}
    assert layout == "gemvfast"
    sc = torch.zeros((8 * zw, N), dtype=torch.float16)
    qz = torch.zeros((8 * zw, N), dtype=torch.float16)
    sc[:G] = s
    qz[:G] = torch.from_numpy(fast_qzeros(case))
    return {"x": x, "qweight": pack_intweight_fast(w.t().contiguous()), "scales": sc, "qzeros": qz}


def fast_qzeros(case):
    """the GEMVFast format's stored zero term fp16(-(s z)) [G, N] (s z is exact in fp32: one rounding)"""
    return (-(case.s.astype(np.float32) * case.z.astype(np.float32))).astype(np.float16)


def _rep(a, g):
    return np.repeat(a, g, axis=0)


def weights_exact(case, layout):
    """[K, N] float64: (w - z) s, or for GEMVFast w s + qzeros with the STORED fp16 qzeros"""
    s = _rep(case.s.astype(np.float64), case.g)
    if layout == "gemvfast":
        return case.w.astype(np.float64) * s + _rep(fast_qzeros(case).astype(np.float64), case.g)
    return (case.w.astype(np.float64) - _rep(case.z.astype(np.float64), case.g)) * s


def rounded_weights(case, layout):
    """[K, N] float16: the reference's dequantised weight, ONE IEEE rounding of the exact value, subnormals kept.  The exact
    value has at most 16 significant bits ((w - z) s: 5 + 11; w s + qzeros: within 2^5 ulps of each other's grid), so the way
    through float32 is exact and numpy's float32 -> float16 conversion is the single round-to-nearest-even."""
    return weights_exact(case, layout).astype(np.float32).astype(np.float16)


def exact(case, layout):
    return case.x.astype(np.float64) @ weights_exact(case, layout)


def exact_rounded(case, layout):
    return case.x.astype(np.float64) @ rounded_weights(case, layout).astype(np.float64)


# ------------------------------------------------------------------ the bound

BATCH_N_P = 4 * 33  # gemv_batch on the GEMV layout: four 32-wide MFMA steps per group


def batch_n_out(wk, passes):
    """gemv_batch on the GEMV layout, from the plan's wk (waves side by side on a tile) and passes over K"""
    return 4 + (wk - 1) + (passes - 1)


def rows_n_out(K):
    return 5 + (K + 2047) // 2048 + 7


def worst_n_out(K, fold):
    return K // fold + 64


def _bias_k(K, biases):
    b = np.empty(K, np.float64)
    b[0::2], b[1::2] = biases
    return b


def _fold_sums(case, layout, fold):
    """sum_f |s_f d_f| [M, N]"""
    M, K, N = case.shape
    F = K // fold
    W = weights_exact(case, layout).reshape(F, fold, N)
    x = case.x.astype(np.float64).reshape(M, F, fold)
    return np.abs(np.einsum("mfk,fkn->mfn", x, W)).sum(1)


def bound(case, layout, kernel, n_out=None, out_scale=None, residual=None, x_slack=None, n_p=None):
    """(want, bound) [M, N] float64 for `kernel`'s arithmetic class.  n_out, n_p: the launch's own depths where the caller knows them;
    out_scale [M]: FX_SCALE's per-row fp32 factor of the fp32 sum; residual [M, N]: FX_RES's second rounding; x_slack [M, K]:
    how far the kernel's own activations may lie from case.x (FX_NORM / gemv_mfma's NORM staging, norm_prologue)."""
    M, K, N = case.shape
    g = case.g
    ax = np.abs(case.x.astype(np.float64))
    moved = 0.0
    if x_slack is not None:
        assert kernel in FACTORISED  # (a norm prologue: gemv_rows' FX_NORM, gemv_mfma's NORM staging)
        ax = ax + x_slack
        moved = x_slack @ np.abs(weights_exact(case, layout))
    if kernel in REF_WEIGHT:
        W16 = rounded_weights(case, layout).astype(np.float64)
        want = case.x.astype(np.float64) @ W16
        return want, ulp16(want) + 1.01 * gamma(K + K // 32 + 64) * (ax @ np.abs(W16))
    fold = min(g, FOLD)
    want = exact(case, layout)
    s = np.abs(_rep(case.s.astype(np.float64), g))
    rows = kernel.startswith("gemv_rows")
    if n_p is None:
        n_p = ROWS_N_P if rows else WORST_N_FOLD
    assert x_slack is None or out_scale is None
    if n_out is None:
        n_out = rows_n_out(K) if rows else worst_n_out(K, fold)
    a_out = _fold_sums(case, layout, fold) + moved
    if kernel in EXACT_INT:
        assert layout == "gemv"
        a_p = ax @ (s * np.abs(case.w.astype(np.float64) - _rep(case.z.astype(np.float64), g)))
        terms = gamma(n_p) * a_p + gamma(n_out) * a_out
    else:
        bk = _bias_k(K, FACTORISED[kernel])[:, None]
        a_p = ax @ (s * (bk + case.w.astype(np.float64)))
        if layout == "gemvfast":
            a_c = ax @ (s * bk + np.abs(_rep(fast_qzeros(case).astype(np.float64), g)))
        else:
            a_c = ax @ (s * (bk + _rep(case.z.astype(np.float64), g)))
        terms = gamma(n_p) * (a_p + a_c) + gamma(n_out) * a_out
    if out_scale is not None:
        sc = np.abs(np.asarray(out_scale, np.float64)).reshape(M, 1)
        want, terms = want * np.asarray(out_scale, np.float64).reshape(M, 1), sc * (terms + U * np.abs(want))
    b = ulp16(want) + 1.01 * terms + (1.0 + 2.0 ** -10) * moved
    if residual is not None:
        r = np.asarray(residual, np.float64)
        want, b = want + r, b + ulp16(want + r) + 2.0 ** -10 * b  # (the sum of two fp16 values rounds once; b moves its argument)
    return want, b


NORM_N = 32        # FX_NORM: e = 1.01 gamma(32) on the value that is rounded to fp16 (docstring)
SILU_SLOPE = 1.1   # max |silu'| = 1.0998 (at x = 2.3994)
SILU_N = 16        # awq_silu_mul_f32's four fp32 operations


def norm_prologue(x, norm_weight, eps, depth=NORM_N):
    """A norm folded into a matmul: (x16 [M, K] float16 = fp16 of the exactly normalised activations, slack [M, K] float64) for an
    implementation whose statistic has `depth` roundings (tests/norm_rope_bound.py counts them; FX_NORM of gemv_rows: NORM_N)"""
    import norm_rope_bound as nrb

    xn = nrb.norm_reference(x, norm_weight, eps)
    lo, hi = nrb.norm_window(xn, depth)
    x16 = xn.astype(np.float16)  # (numpy rounds float64 to float16 once, to nearest even)
    mid = x16.astype(np.float64)
    return x16, np.maximum(hi - mid, mid - lo)


def silu(v):
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def silu_pairs_bound(want, b):
    """FX_PAIRS: (want, bound) [M, N / 2] of silu(gate) up from the plain (want, bound) [M, N], columns (2 i, 2 i + 1) = (gate_i, up_i)"""
    G, U, bg, bu = want[:, 0::2], want[:, 1::2], b[:, 0::2], b[:, 1::2]
    S = silu(G)
    out = S * U
    e1 = (np.abs(S) + SILU_SLOPE * bg) * bu + SILU_SLOPE * np.abs(U) * bg
    e2 = e1 + gamma(SILU_N) * (np.abs(out) + e1)
    return out, ulp16(out) + (1.0 + 2.0 ** -10) * e2


def assert_within(y, want, bnd, what=""):
    """|y - want| <= bnd element by element (NaN fails); the message names indices, value, reference and error / bound"""
    y = np.asarray(y, np.float64)
    err = np.abs(y - want)
    bad = ~(err <= bnd)
    if bad.any():
        ratio = np.where(np.isnan(err), np.inf, err / bnd)
        order = np.argsort(-ratio, axis=None)[:8]
        where = ", ".join(f"{tuple(int(v) for v in np.unravel_index(i, y.shape))}: {y.flat[i]:.6g} vs {want.flat[i]:.6g} "
                          f"(err {err.flat[i]:.3g} = {ratio.flat[i]:.3g} x bound {bnd.flat[i]:.3g})" for i in order)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} outside the derived bound; worst at {where}")


def worst(y, want, bnd):
    """(largest err / bound, largest error in fp16 ulps of the output)"""
    err = np.abs(np.asarray(y, np.float64) - want)
    return float((err / bnd).max()), float((err / ulp16(want)).max())


# ------------------------------------------------------------------ inputs

def _few_bit_scales(rng, G, N):
    """fp16 scales j 2^-11, 10 <= j < 50 (0.005 .. 0.024): six significant bits, so that s z is exact in fp16 and the GEMVFast
    format's stored zero term carries no rounding of its own"""
    return (rng.integers(10, 50, (G, N)) * 2.0 ** -11).astype(np.float16)


def make_case(regime, K, N, g, M, layout="gemv", seed=0):
    """Seeded adversarial operands.  Every value is fp16-representable; every exact output is finite and below 60000."""
    assert regime in REGIMES and K % g == 0
    rng = np.random.default_rng([seed, K, N, g, REGIMES.index(regime)])
    G = K // g
    w = rng.integers(0, 16, (K, N)).astype(np.uint8)
    z = rng.integers(0, 16, (G, N)).astype(np.uint8)
    s = (rng.random((G, N)) * 0.02 + 0.005).astype(np.float16)
    biased = (np.abs(rng.standard_normal((M, K))) + 0.5).astype(np.float16)
    if regime == "biased":
        x = biased
    elif regime == "outlier":
        x = rng.standard_normal((M, K)).astype(np.float16)
        for m in range(M):
            k0 = int(rng.integers(0, K))
            x[m, k0] = np.float16(512.0 if m % 2 == 0 else -512.0)
            w[k0, 0::4] = z[k0 // g, 0::4]  # a quarter of the columns: the outlier meets w == z
    elif regime == "flat":
        x = biased
        s = _few_bit_scales(rng, G, N)
        w[:, 0::4] = _rep(z, g)[:, 0::4]     # whole columns of w == z: the exact output is 0
        w[:, 1::4], z[:, 1::4] = 15, 0
        w[:, 2::4], z[:, 2::4] = 0, 15
    elif regime == "scales":
        # a column alternates between the two scales of a pair from group to group (random phase): neighbours differ by 2^6 or
        # more, or one of them is 0 or negative -- a scale or zero point taken from the neighbouring group is a gross error
        pairs = np.array([[2.0 ** -20, 2.0 ** -14], [2.0 ** -16, -0.01], [0.0, 0.01], [0.01, 8.0], [2.0 ** -14, 8.0], [-0.01, 8.0],
                          [2.0 ** -20, 0.01], [2.0 ** -16, 2.0 ** -10]])
        pick = (np.arange(N) + int(rng.integers(0, 8))) % len(pairs)
        phase = rng.integers(0, 2, N)
        s = pairs[pick[None, :], (np.arange(G)[:, None] + phase[None, :]) % 2].astype(np.float16)
        x = (0.5 * rng.standard_normal((M, K))).astype(np.float16)
    else:  # cancel: groups in pairs with the same weights and opposite activations; each group's term is large, the sum ~ 0
        w = rng.integers(8, 16, (K, N)).astype(np.uint8)
        z = rng.integers(0, 4, (G, N)).astype(np.uint8)
        x = biased.copy().reshape(M, G, g)
        for j in range(0, G - 1, 2):
            w[(j + 1) * g:(j + 2) * g] = w[j * g:(j + 1) * g]
            z[j + 1], s[j + 1] = z[j], s[j]
            x[:, j + 1] = -x[:, j]
        if G % 2:  # the group without a partner: half a group each way
            x[:, G - 1, g // 2:] = -x[:, G - 1, :g // 2]
            w[(G - 1) * g + g // 2:] = w[(G - 1) * g:(G - 1) * g + g // 2]
        x = x.reshape(M, K)
    case = Case(np.ascontiguousarray(x), w, z, s, g, regime)
    y = exact(case, layout)
    assert np.isfinite(y).all() and np.abs(y).max() < 60000.0, (regime, K, N, g, M, float(np.abs(y).max()))
    return case
