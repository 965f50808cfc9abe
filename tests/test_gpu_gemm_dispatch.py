"""What a GEMM-layout call launches, through `ops.gemm_forward` (and, for the fused entries, `ops.gemm_forward_normed` and
`ops.gemm_forward_ex`): for every shape, row count and kernel field below, the error code (0 for a call that succeeds) and
`ops.last_kernel()` after the call, against a literal table.  The table was recorded on an MI355X from the library and wrappers as
they stood BEFORE the host path was folded onto one checker, one argument fill and one dispatch (csrc/capi.hip, ops.py), so it pins
the dispatch policy -- AUTO and explicit, and AUTO's two run-time fallthroughs -- from outside.  Every call that succeeds is also held
to the oracle with the bounds of tests/test_gpu_parity.py's test_gemm_vs_oracle_all_variants: the reference-order kernels to the
product bound, the MFMA decode kernel to the bound widened by the reference's own weight-rounding noise AND to the exact product.

The shapes are the smallest that reach every branch (found with the host query awq_gemm_auto_kernel, checked below): 256 x 256 in
groups of 128 (AUTO: the decode kernel up to 8 rows, the batched kernel before it at 9 .. 16 and up to 64, the LDS-tiled kernel
beyond), 256 x 264 (N % 32: the naive kernel at decode sizes), 64 x 1024 in groups of 64 (K < 128: the batched kernel refuses, so
the decode kernel keeps 9 .. 16 rows and the tiled kernel starts at 17; at 8192 rows its 64 x 4 tiles of 128 x 256 reach the
register-decoded prefill kernel).  AUTO's fallthrough from the batched to the tiled kernel needs more than 512 (slice, tile) pairs
at M > 32 -- K > 8192 with N = 16384: 9216 x 16384 at 33 rows, a test of its own.  `last_kernel` is per thread and survives a
refused call, so the calls of a shape run in one fixed order, a successful one first."""
import numpy as np
import pytest
import torch

from conftest import assert_close_to_exact, assert_product_close
from test_gpu_parity import fullrange_case

pytestmark = pytest.mark.gpu

NAIVE, VALU, MFMA_GEMV, TILED, REGB, SKINNY = 1, 2, 3, 4, 5, 6
SHAPES = [(256, 256, 128), (256, 264, 128), (64, 1024, 64)]  # (K, N, group_size)
ROWS = [1, 4, 8, 9, 16, 17, 64, 65]
KERNELS = [0, NAIVE, VALU, MFMA_GEMV, TILED, REGB, SKINNY, 9]  # the kernel field: AUTO, every AWQ_GEMM_KERNEL_*, an unknown one
# what awq_gemm_auto_kernel answers for ROWS (the run-time table below has to agree wherever AUTO's first choice runs)
AUTO = ["3 3 3 6 6 6 6 4", "1 1 1 6 6 6 6 4", "3 3 3 3 3 4 4 4"]
NAMES = {NAIVE: "naive", MFMA_GEMV: "gemv_mfma", TILED: "gemm_tiled", REGB: "gemm_regb", SKINNY: "gemm_skinny"}

# EXPECTED[shape][M]: one entry per kernel field of KERNELS, "<last_kernel>" or "<code>/<last_kernel>"
EXPECTED = [
    {
        1: "gemv_mfma naive gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        4: "gemv_mfma naive gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        8: "gemv_mfma naive -3/gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        9: "gemm_skinny naive -3/gemv_valu gemv_mfma gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        16: "gemm_skinny naive -3/gemv_valu gemv_mfma gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        17: "gemm_skinny naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        64: "gemm_skinny naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        65: "gemm_tiled naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
    },
    {
        1: "naive naive -3/gemv_valu -3/gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        4: "naive naive -3/gemv_valu -3/gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        8: "naive naive -3/gemv_valu -3/gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        9: "gemm_skinny naive -3/gemv_valu -3/gemv_mfma gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        16: "gemm_skinny naive -3/gemv_valu -3/gemv_mfma gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        17: "gemm_skinny naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        64: "gemm_skinny naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb gemm_skinny -3/gemm_skinny",
        65: "gemm_tiled naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
    },
    {
        1: "gemv_mfma naive gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        4: "gemv_mfma naive gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        8: "gemv_mfma naive -3/gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        9: "gemv_mfma naive -3/gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        16: "gemv_mfma naive -3/gemv_valu gemv_mfma gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        17: "gemm_tiled naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        64: "gemm_tiled naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
        65: "gemm_tiled naive -3/gemv_valu -3/gemv_valu gemm_tiled gemm_regb -3/gemm_skinny -3/gemm_skinny",
    },
]
# 8192 rows of the third shape: AUTO, the prefill kernel and the tiled kernel by name
PREFILL_ROWS, PREFILL_KERNELS = 8192, [0, REGB, TILED]
PREFILL_EXPECTED = "gemm_regb gemm_regb gemm_tiled"
# 33 rows of 9216 x 16384: the batched kernel is AUTO's first choice, its launcher refuses (nine slices of 64 tiles do not fit the
# exchange region) and the tiled kernel runs; named, the batched kernel is not replaced
WIDE, WIDE_ROWS, WIDE_KERNELS = (9216, 16384, 128), 33, [0, SKINNY]
WIDE_EXPECTED = "gemm_tiled -3/gemm_skinny"
# the fused entries on the first shape: (entry, rows, flags) in call order after one naive call ("naive": another in between)
X_GATED = 1 << 18
FUSED = [("normed", 5, 0), ("normed", 1, 0), ("normed", 4, 0), ("normed", 1, X_GATED), ("normed", 1, TILED), ("naive", 1, NAIVE),
         ("ex", 5, 0), ("ex", 1, 0), ("ex", 4, 0), ("ex", 1, X_GATED), ("ex", 1, SKINNY)]
FUSED_EXPECTED = "-3/naive gemv_mfma gemv_mfma -3/gemv_mfma -3/gemv_mfma naive -3/naive gemv_mfma gemv_mfma -3/gemv_mfma -3/gemv_mfma"


def check_product(ops, y, x, qw, qz, s, g, bias, ref, what):
    """the bound of test_gemm_vs_oracle_all_variants for the kernel that ran; ref = (y32, wsigma, yex) of all rows"""
    M = y.shape[0]
    yn = y.cpu().numpy().astype(np.float64)
    if ops.last_kernel() == "gemv_mfma":  # exact integer dot product, scale applied in fp32
        assert_product_close(yn, ref[0][:M], what, wsigma=ref[1][:M])
        assert_close_to_exact(yn, ref[2][:M], what)
    else:  # reference-order numerics: fp16-rounded weights
        assert_product_close(yn, ref[0][:M], what)


def reference(oracle, x, qw, qz, s, g, bias, exact=True):
    a = [t.numpy() for t in (x, qw, qz, s)]
    y32, _ = oracle.linear_gemm(*a, g, bias.numpy())
    if not exact:
        return y32, None, None
    return y32, oracle.weight_rounding_sigma(a[0], oracle.dequant_gemm(a[1], a[2], a[3], g)), oracle.linear_gemm_exact(*a, g, bias.numpy())


def observe(ops, x, qw, qz, s, bias, rows, kernels, check):
    """["<code>/<last_kernel>" per (M, kernel field)] in call order; check(y, what) for every call that succeeds"""
    from autoawq_amd import _lib

    dx, dq, dz, ds, db = x.cuda(), qw.cuda(), qz.cuda(), s.cuda(), bias.cuda()
    seen = []
    for M in rows:
        for kern in kernels:
            code = 0
            try:
                y = ops.gemm_forward(dx[:M], dq, ds, dz, db, flags=ops.gemm_flags(kernel=kern))
            except _lib.AwqHipError as e:
                code = e.code
            seen.append((f"{code}/" if code else "") + ops.last_kernel())
            if code == 0:
                check(y, f"K{x.shape[1]} N{y.shape[1]} M{M} kernel {kern}")
    return seen


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_dispatch_table(oracle, shape):
    from autoawq_amd import ops

    K, N, g = SHAPES[shape]
    assert [ops.auto_kernel(M, K, N, g) for M in ROWS] == [int(k) for k in AUTO[shape].split()]
    qw, qz, s, x, bias = fullrange_case(K, N, g, max(ROWS), seed=K + N, realistic=(N % 64 == 0))
    ref = reference(oracle, x, qw, qz, s, g, bias)  # all rows, once (a row's result does not depend on the others)
    seen = observe(ops, x, qw, qz, s, bias, ROWS, KERNELS, lambda y, what: check_product(ops, y, x, qw, qz, s, g, bias, ref, what))
    assert ops.workspace_is_clean(torch.device("cuda", torch.cuda.current_device()))
    want = EXPECTED[shape]
    rows = {M: seen[i * len(KERNELS):(i + 1) * len(KERNELS)] for i, M in enumerate(ROWS)}
    for M, got in rows.items():
        print(SHAPES[shape], M, " ".join(got))
    assert sorted(want) == ROWS
    for M, got in rows.items():
        assert got == want[M].split(), (SHAPES[shape], M, dict(zip(KERNELS, got)))
        first = NAMES[ops.auto_kernel(M, K, N, g)]
        assert got[0] == first, (SHAPES[shape], M)  # no fallthrough on these shapes: AUTO runs what the host query names


def test_dispatch_prefill_rows(oracle):
    from autoawq_amd import ops

    K, N, g = SHAPES[2]
    assert (PREFILL_ROWS + 127) // 128 * ((N + 255) // 256) >= 256 and ops.auto_kernel(PREFILL_ROWS, K, N, g) == REGB
    qw, qz, s, x, bias = fullrange_case(K, N, g, PREFILL_ROWS, seed=K + N, realistic=True)
    ref = reference(oracle, x, qw, qz, s, g, bias, exact=False)
    seen = observe(ops, x, qw, qz, s, bias, [PREFILL_ROWS], PREFILL_KERNELS, lambda y, what: check_product(ops, y, x, qw, qz, s, g, bias, ref, what))
    print("prefill", " ".join(seen))
    assert seen == PREFILL_EXPECTED.split()


def test_dispatch_falls_through_from_the_batched_to_the_tiled_kernel(oracle):
    from autoawq_amd import ops

    K, N, g = WIDE
    assert ops.auto_kernel(WIDE_ROWS, K, N, g) == SKINNY
    qw, qz, s, x, bias = fullrange_case(K, N, g, WIDE_ROWS, seed=K + N, realistic=True)
    ref = reference(oracle, x, qw, qz, s, g, bias, exact=False)
    seen = observe(ops, x, qw, qz, s, bias, [WIDE_ROWS], WIDE_KERNELS, lambda y, what: check_product(ops, y, x, qw, qz, s, g, bias, ref, what))
    print("wide", " ".join(seen))
    assert seen == WIDE_EXPECTED.split()


def test_fused_entries(oracle):
    """awq_gemm_forward_normed / awq_gemm_forward_ex (with a norm weight): the decode kernel at one and four rows, held to the oracle's
    product of the reference RMSNorm's rows; refused at five rows, with gated activations beside the norm, and with a kernel field
    that names another kernel -- `last_kernel` stays what the last launch left"""
    from autoawq_amd import _lib, ops
    from oracle import decoder_oracle

    K, N, g = SHAPES[0]
    qw, qz, s, x, bias = fullrange_case(K, N, g, 5, seed=K + N + 1, realistic=True)
    w = (torch.rand(K, generator=torch.Generator().manual_seed(3)) + 0.5).half()
    xn = torch.from_numpy(decoder_oracle.rmsnorm_reference(x.numpy(), w.numpy(), 1e-5))
    ref = reference(oracle, xn, qw, qz, s, g, bias)
    dx, dq, dz, ds, db, dw = x.cuda(), qw.cuda(), qz.cuda(), s.cuda(), bias.cuda(), w.cuda()
    ops.gemm_forward(dx[:1], dq, ds, dz, db, flags=NAIVE)
    seen = []
    for entry, M, flags in FUSED:
        code = 0
        xin = torch.cat([dx[:M], dx[:M]], 1) if entry == "ex" and flags & X_GATED else dx[:M]  # [gate | up]: 2 K halves a row
        try:
            if entry == "normed":
                y, _ = ops.gemm_forward_normed(xin, dw, 1e-5, dq, ds, dz, db, flags=flags)
            elif entry == "ex":
                y, _ = ops.gemm_forward_ex(xin, dq, ds, dz, db, flags=flags, norm_weight=dw, norm_eps=1e-5)
            else:
                ops.gemm_forward(xin, dq, ds, dz, db, flags=flags)
                seen.append(ops.last_kernel())
                continue
        except _lib.AwqHipError as e:
            code = e.code
        seen.append((f"{code}/" if code else "") + ops.last_kernel())
        if code == 0:
            check_product(ops, y, xn, qw, qz, s, g, bias, ref, f"{entry} M{M}")
    print("fused", " ".join(seen))
    assert seen == FUSED_EXPECTED.split()
