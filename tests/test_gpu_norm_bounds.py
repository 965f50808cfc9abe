"""RMSNorm, all four implementations, element by element against the float64 reference and the window derived from each
implementation's own arithmetic (tests/norm_rope_bound.py): Gaussian rows, quiet rows whose mean square is near or far below eps
(`tiny`, `subnormal` -- where a wrong eps shows), an outlier of 65504, rows of huge values, an all-zero row, NaN / inf rows; weights
of both signs with exact zeros and values that overflow fp16; eps = 1e-5 and 1e-6.  The norms folded into a matmul (gemv_mfma's
NORM staging with and without the producer's statistic, FX_NORM of gemv_rows) are held to the matmul bound of
tests/matmul_bound.py with the window as slack on the activations.

NORM_ROPE_BOUND_RECORD=<file>: every case appends "implementation shape kind eps ratio" (recorded, not asserted)."""
import numpy as np
import pytest
import torch

import matmul_bound as mb
import norm_rope_bound as nrb

pytestmark = pytest.mark.gpu

BAD_SHAPE = -1  # AWQ_ERR_BAD_SHAPE (include/awq_hip.h)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint16)


def same_stream(got, want16):
    """bit for bit; a NaN may carry any payload (numpy and the fp32 -> fp16 conversion of the device choose their own)"""
    g, w = bits(got), bits(want16)
    both_nan = np.isnan(g.view(np.float16)) & np.isnan(w.view(np.float16))
    return bool(((g == w) | both_nan).all())


_weights = {}


def weights(K, N, g, layout, seed):
    """(logical case, device buffers) of a weight matrix, made once per shape (`biased` of matmul_bound: the plain recipe)"""
    key = (K, N, g, layout, seed)
    if key not in _weights:
        case = mb.make_case("biased", K, N, g, 4, layout, seed=seed)
        _weights[key] = (case, {k: v.cuda() for k, v in mb.pack(case, layout).items()})
    return _weights[key]


# ------------------------------------------------------------------ awq_rmsnorm_kernel

@pytest.mark.parametrize("M", nrb.RMSNORM_M)
@pytest.mark.parametrize("H", nrb.RMSNORM_H)
def test_rmsnorm_window(ops, M, H):
    depth = nrb.depth_rmsnorm(H)
    w = nrb.norm_weights(H, 3)
    wd = dev(w)
    for kind in nrb.NORM_KINDS + ("nonfinite",):
        if kind == "nonfinite":
            x, r = nrb.norm_nonfinite(M, H, 3)
            h = x
        else:
            h = nrb.norm_rows(kind, M, H, 3)
            x, r = nrb.split_rows(h, 3)
        for eps in nrb.EPSS:
            y = nrb.norm_reference(h, w, eps)
            lo, hi = nrb.norm_window(y, depth)
            got = ops.rmsnorm(dev(h), wd, eps).cpu().numpy()
            nrb.record("rmsnorm", f"M{M} H{H}", kind, eps, nrb.worst_ratio(got, y, lo, hi))
            nrb.assert_in_window(got, lo, hi, f"rmsnorm {kind} M{M} H{H} eps {eps}")
            # residual form: the stream is fp16(x + r) bit for bit, and the norm is the norm of that
            y, hh = nrb.norm_reference(x, w, eps, r)
            lo, hi = nrb.norm_window(y, depth)
            rd = dev(r)
            got = ops.rmsnorm(dev(x), wd, eps, residual=rd).cpu().numpy()
            assert same_stream(rd, hh) if kind == "nonfinite" else np.array_equal(bits(rd), bits(hh)), (kind, M, H)
            nrb.record("add_rmsnorm", f"M{M} H{H}", kind, eps, nrb.worst_ratio(got, y, lo, hi))
            nrb.assert_in_window(got, lo, hi, f"rmsnorm + residual {kind} M{M} H{H} eps {eps}")
            if kind == "nonfinite":  # (what the window already says, spelt out: a NaN row, 0 / NaN around an inf)
                assert np.isnan(got[0]).all() and (M == 1 or (np.isnan(got[1]).sum() == 1 and not np.nan_to_num(got[1:3]).any()))


@pytest.mark.parametrize("H", [16392, 12])
def test_rmsnorm_refuses(ops, H):
    from autoawq_amd import _lib

    x = torch.zeros((2, H), dtype=torch.float16, device="cuda")
    out = torch.full((2, H), 7.0, dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.AwqHipError) as e:
        ops.rmsnorm(x, torch.ones(H, dtype=torch.float16, device="cuda"), 1e-5, out=out)
    assert e.value.code == BAD_SHAPE
    assert bool((out == 7.0).all())  # nothing was launched


# ------------------------------------------------------------------ gemv_mfma's NORM staging (awq_gemm_forward_normed)

def normed_bound(h16, nw, eps, depth, wcase, g, kind, kernel="gemv_mfma", layout="gemm", **kw):
    x16, slack = mb.norm_prologue(h16, nw, eps, depth)
    return mb.bound(mb.Case(x16, wcase.w, wcase.z, wcase.s, g, kind), layout, kernel, x_slack=slack, **kw)


@pytest.mark.parametrize("M", nrb.MFMA_NORM_M)
@pytest.mark.parametrize("K,N,g", nrb.MFMA_NORM_SHAPES)
def test_norm_folded_into_projection_bound(ops, M, K, N, g):
    wcase, d = weights(K, N, g, "gemm", 7)
    depth = nrb.depth_mfma_norm(K)
    nw = nrb.norm_weights(K, 3, big=False)
    nwd = dev(nw)
    for kind in nrb.MFMA_NORM_KINDS:
        h = nrb.norm_rows(kind, M, K, 3)
        x, r = nrb.split_rows(h, 3)
        for eps in nrb.EPSS:
            for res in (None, r):
                src = h if res is None else x
                got, stream = ops.gemm_forward_normed(dev(src), nwd, eps, d["qweight"], d["scales"], d["qzeros"],
                                                      residual=None if res is None else dev(res))
                assert ops.last_kernel() == "gemv_mfma"
                hh = h if res is None else nrb.stream_sum(x, r)
                assert (stream is None) if res is None else np.array_equal(bits(stream), bits(hh))
                want, bnd = normed_bound(hh, nw, eps, depth, wcase, g, kind)
                y = got.cpu().numpy().astype(np.float64)
                nrb.record("gemm_forward_normed" + ("" if res is None else "+res"), f"M{M} K{K} N{N} g{g}", kind, eps, mb.worst(y, want, bnd)[0])
                mb.assert_within(y, want, bnd, f"gemm_forward_normed {kind} M{M} K{K} g{g} eps {eps} residual {res is not None}")


# ------------------------------------------------------------------ the statistic hand-over (awq_gemm_forward_ex: ssq_out -> ssq_in)

@pytest.mark.parametrize("M", nrb.SSQ_M)
@pytest.mark.parametrize("I,H,g", nrb.SSQ_SHAPES)
def test_statistic_hand_over_bound(ops, M, I, H, g):
    """The producer's per-tile sums of squares against the float64 sums of the stream it RETURNED, within gamma(depth) of each;
    the stream itself within the matmul bound with the residual's second rounding; the consumer's product within the matmul
    bound with the window of the tile sum's depth as slack."""
    c1, d1 = weights(I, H, g, "gemm", 7)     # the producing projection: I -> H
    c2, d2 = weights(H, 256, g, "gemm", 8)   # the next one: H -> 256
    nw = nrb.norm_weights(H, 3, big=False)
    tiles = (H + 255) // 256
    for kind in nrb.SSQ_KINDS:
        amp = 1.0 if kind == "normal" else 2.0 ** -10   # (the projection of a tiny row is tiny: |W| ~ 0.1, sqrt(I) ~ 16)
        x = (amp * np.random.default_rng([M, I, H]).standard_normal((M, I))).astype(np.float16)
        hres = nrb.norm_rows(kind, M, H, 3)
        stream, ssq = ops.gemm_forward_ex(dev(x), d1["qweight"], d1["scales"], d1["qzeros"], add_residual=dev(hres), want_ssq=True)
        assert ops.last_kernel() == "gemv_mfma"
        s16 = stream.cpu().numpy()
        want, bnd = mb.bound(mb.Case(x, c1.w, c1.z, c1.s, g, kind), "gemm", "gemv_mfma", residual=hres.astype(np.float64))
        mb.assert_within(s16.astype(np.float64), want, bnd, f"residual epilogue {kind} M{M} I{I} H{H}")
        want_ssq = nrb.ssq_tiles_reference(s16)
        got_ssq = ssq.cpu().numpy().astype(np.float64)
        assert got_ssq.shape == (M, tiles)
        err = np.abs(got_ssq - want_ssq)
        nrb.record("ssq_out", f"M{M} H{H}", kind, 0.0, float((err / (nrb.gamma(nrb.SSQ_TILE_N) * want_ssq)).max()))
        assert (err <= nrb.gamma(nrb.SSQ_TILE_N) * want_ssq).all(), (kind, M, H, float((err / want_ssq).max()))
        for eps in nrb.EPSS:
            nxt, none = ops.gemm_forward_ex(stream, d2["qweight"], d2["scales"], d2["qzeros"], norm_weight=dev(nw), norm_eps=eps, ssq_in=ssq)
            assert none is None and ops.last_kernel() == "gemv_mfma"
            want, bnd = normed_bound(s16, nw, eps, nrb.depth_mfma_ssq(), c2, g, kind)
            y = nxt.cpu().numpy().astype(np.float64)
            nrb.record("gemm_forward_ex(ssq_in)", f"M{M} H{H} g{g}", kind, eps, mb.worst(y, want, bnd)[0])
            mb.assert_within(y, want, bnd, f"ssq_in consumer {kind} M{M} H{H} eps {eps}")
    assert ops.workspace_is_clean(torch.device("cuda", torch.cuda.current_device()))


# ------------------------------------------------------------------ FX_NORM of gemv_rows (awq_gemv_forward_ex)

@pytest.mark.parametrize("form", ["norm", "norm_res", "norm_pairs"])
@pytest.mark.parametrize("K,N,g", nrb.ROWS_NORM_SHAPES)
def test_gemv_rows_norm_forms_on_quiet_rows(ops, K, N, g, form):
    """test_gpu_matmul_bounds.py::test_gemv_rows_fx_forms' norm forms on `tiny` and `subnormal` activations, both eps, also at the
    largest K the prologue takes"""
    wcase, d = weights(K, N, g, "gemv", 7)
    nw = nrb.norm_weights(K, 3, big=False)
    res = (4.0 * np.random.default_rng(5).standard_normal((1, N))).astype(np.float16)
    for kind in nrb.ROWS_NORM_KINDS:
        h = nrb.norm_rows(kind, 1, K, 3)
        for eps in nrb.EPSS:
            kw = {"norm_weight": dev(nw), "norm_eps": eps}
            if "res" in form:
                kw["add_residual"] = dev(res)
            if "pairs" in form:
                kw["silu_pairs"] = True
            y = ops.gemv_forward_ex(dev(h), d["qweight"], d["scales"], d["qzeros"], g, **kw).cpu().numpy().astype(np.float64)
            assert ops.last_kernel() == "gemv_rows"
            want, bnd = normed_bound(h, nw, eps, mb.NORM_N, wcase, g, kind, kernel="gemv_rows", layout="gemv",
                                     residual=res.astype(np.float64) if "res" in form else None)
            if "pairs" in form:
                want, bnd = mb.silu_pairs_bound(want, bnd)
            assert y.shape == want.shape
            nrb.record(f"gemv_forward_ex({form})", f"K{K} N{N} g{g}", kind, eps, mb.worst(y, want, bnd)[0])
            mb.assert_within(y, want, bnd, f"gemv_rows fx {form} {kind} K{K} N{N} eps {eps}")
