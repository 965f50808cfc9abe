"""What a GEMV- or GEMVFast-layout call launches, through the `ops` wrappers: for every shape, row count and kernel field below, the
error code (0 for a call that succeeds) and `ops.last_kernel()` after the call, against a literal table.  The table was recorded on an
MI355X from the library and wrappers as they stood BEFORE the host path was folded onto one argument struct, one checker and one
dispatch per layout (csrc/capi.hip, ops.py), so it pins the dispatch policy -- AUTO and explicit, the wrappers' single call / row
chunks, the fallthrough on GEMVFast -- from outside.  Every call that succeeds is also held to the oracle with the bound of
tests/test_gpu_parity.py's test_gemv_layout_vs_oracle and its GEMVFast twin.

The shapes are the smallest that reach every branch: K = 256 (below every threshold), 4096 (the row-streaming kernel up to four
rows; GEMVFast: one pass of eight waves, the batched kernel at every M), 8192 (the batched kernel from three rows) and a group size
of 64, which the batched and row-streaming kernels refuse (the LDS and tile kernels).  `last_kernel` is per thread and survives a
refused call, so the calls of a shape run in one fixed order, a successful one first."""
import numpy as np
import pytest
import torch

from conftest import assert_product_close
from test_gpu_parity import gemv_case, gemvfast_case

pytestmark = pytest.mark.gpu

SHAPES = [(256, 64, 128), (4096, 64, 128), (8192, 64, 128), (1024, 8192, 64)]  # (K, N, group_size)
ROWS = [1, 2, 3, 4, 5, 16, 17, 33, 129, 257]
KERNELS = {"gemv": [0, 1, 2, 3, 4, 5, 7], "gemvfast": [0, 1, 5]}  # the kernel field: AUTO, every AWQ_GEMV_KERNEL_*, an unknown one

# EXPECTED[layout][shape][M]: one entry per kernel field of KERNELS[layout], "<last_kernel>" or "<code>/<last_kernel>"
EXPECTED = {
    "gemv": [
        {
            1: "gemv_rows gemv_nk gemv_rows -3/gemv_rows gemm_regb_nk gemv_batch gemv_nk",
            2: "gemv_rows gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            3: "gemv_rows gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            4: "gemv_rows gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            5: "gemv_batch gemv_nk -3/gemv_nk gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            16: "gemv_batch gemv_nk -3/gemv_nk gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            17: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            33: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            129: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            257: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_lds gemm_regb_nk gemv_batch gemv_nk",
        },
        {
            1: "gemv_rows gemv_nk gemv_rows -3/gemv_rows gemm_regb_nk gemv_batch gemv_nk",
            2: "gemv_rows gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            3: "gemv_rows gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            4: "gemv_batch gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            5: "gemv_batch gemv_nk -3/gemv_nk gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            16: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            17: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            33: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            129: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            257: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
        },
        {
            1: "gemv_rows gemv_nk gemv_rows -3/gemv_rows gemm_regb_nk gemv_batch gemv_nk",
            2: "gemv_rows gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            3: "gemv_batch gemv_nk gemv_rows gemv_lds gemm_regb_nk gemv_batch gemv_nk",
            4: "gemv_batch gemv_nk gemv_rows -3/gemv_rows gemm_regb_nk gemv_batch gemv_nk",
            5: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            16: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            17: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            33: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            129: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
            257: "gemv_batch gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk gemv_batch gemv_nk",
        },
        {
            1: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            2: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            3: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            4: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            5: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            16: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            17: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            33: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            129: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
            257: "gemv_nk gemv_nk -3/gemv_nk -3/gemv_nk gemm_regb_nk -3/gemm_regb_nk gemv_nk",
        },
    ],
    "gemvfast": [
        {
            1: "gemv_fast gemv_fast gemv_batch_fast",
            2: "gemv_fast gemv_fast gemv_batch_fast",
            3: "gemv_fast gemv_fast gemv_batch_fast",
            4: "gemv_fast gemv_fast gemv_batch_fast",
            5: "gemv_batch_fast gemv_fast gemv_batch_fast",
            16: "gemv_batch_fast gemv_fast gemv_batch_fast",
            17: "gemv_batch_fast gemv_fast gemv_batch_fast",
            33: "gemv_batch_fast gemv_fast gemv_batch_fast",
            129: "gemv_batch_fast gemv_fast gemv_batch_fast",
            257: "gemv_batch_fast gemv_fast gemv_batch_fast",
        },
        {
            1: "gemv_batch_fast gemv_fast gemv_batch_fast",
            2: "gemv_batch_fast gemv_fast gemv_batch_fast",
            3: "gemv_batch_fast gemv_fast gemv_batch_fast",
            4: "gemv_batch_fast gemv_fast gemv_batch_fast",
            5: "gemv_batch_fast gemv_fast gemv_batch_fast",
            16: "gemv_batch_fast gemv_fast gemv_batch_fast",
            17: "gemv_batch_fast gemv_fast gemv_batch_fast",
            33: "gemv_batch_fast gemv_fast gemv_batch_fast",
            129: "gemv_batch_fast gemv_fast gemv_batch_fast",
            257: "gemv_batch_fast gemv_fast gemv_batch_fast",
        },
        {
            1: "gemv_fast gemv_fast gemv_batch_fast",
            2: "gemv_fast gemv_fast gemv_batch_fast",
            3: "gemv_fast gemv_fast gemv_batch_fast",
            4: "gemv_fast gemv_fast gemv_batch_fast",
            5: "gemv_batch_fast gemv_fast gemv_batch_fast",
            16: "gemv_batch_fast gemv_fast gemv_batch_fast",
            17: "gemv_batch_fast gemv_fast gemv_batch_fast",
            33: "gemv_batch_fast gemv_fast gemv_batch_fast",
            129: "gemv_batch_fast gemv_fast gemv_batch_fast",
            257: "gemv_batch_fast gemv_fast gemv_batch_fast",
        },
        {
            1: "gemv_fast gemv_fast -3/gemv_fast",
            2: "gemv_fast gemv_fast -3/gemv_fast",
            3: "gemv_fast gemv_fast -3/gemv_fast",
            4: "gemv_fast gemv_fast -3/gemv_fast",
            5: "gemv_fast gemv_fast -3/gemv_fast",
            16: "gemv_fast gemv_fast -3/gemv_fast",
            17: "gemv_fast gemv_fast -3/gemv_fast",
            33: "gemv_fast gemv_fast -3/gemv_fast",
            129: "gemv_fast gemv_fast -3/gemv_fast",
            257: "gemv_fast gemv_fast -3/gemv_fast",
        },
    ],
}


def case(layout, K, N, g):
    """(qweight, scales, qzeros, x) of the layout, on the host, in the wrappers' argument order"""
    if layout == "gemv":
        qw, qz, sc, x = gemv_case(K, N, g, max(ROWS), seed=K + N)
    else:
        qw, sc, qz, x = gemvfast_case(K, N, g, max(ROWS), seed=K + N)
    return qw, sc, qz, x


def observe(ops, layout, g, qw, sc, qz, x, check=None):
    """{M: ["<code>/<last_kernel>" per kernel field]} in call order; check(y, M, what) for every call that succeeds"""
    from autoawq_amd import _lib

    forward = ops.gemv_forward if layout == "gemv" else ops.gemv_fast_forward
    qw, sc, qz, x = qw.cuda(), sc.cuda(), qz.cuda(), x.cuda()
    seen = {}
    for M in ROWS:
        for kern in KERNELS[layout]:
            code = 0
            try:
                y = forward(x[:M], qw, sc, qz, g, flags=ops.gemm_flags(kernel=kern))
            except _lib.AwqHipError as e:
                code = e.code
            seen.setdefault(M, []).append((f"{code}/" if code else "") + ops.last_kernel())
            if code == 0 and check is not None:
                check(y.cpu().numpy().astype(np.float64), M, f"{layout} K{x.shape[1]} N{y.shape[1]} g{g} M{M} kernel {kern}")
    return seen


@pytest.mark.parametrize("layout", ["gemv", "gemvfast"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_dispatch_table(oracle, layout, shape):
    from autoawq_amd import ops

    K, N, g = SHAPES[shape]
    qw, sc, qz, x = case(layout, K, N, g)
    # the oracle's product of all rows, once (a row's result does not depend on the others)
    W = (oracle.dequant_gemv(qw.numpy(), qz.numpy(), sc.numpy(), g) if layout == "gemv" else
         oracle.dequant_gemvfast(qw.numpy(), sc.numpy(), qz.numpy(), g))
    y32, _ = oracle.matmul(x.numpy(), W)
    wsig = oracle.weight_rounding_sigma(x.numpy(), W)
    seen = observe(ops, layout, g, qw, sc, qz, x, lambda y, M, what: assert_product_close(y, y32[:M], what, wsigma=wsig[:M]))
    want = EXPECTED[layout][shape]
    assert sorted(want) == ROWS
    for M in ROWS:
        print(layout, SHAPES[shape], M, " ".join(seen[M]))
        assert seen[M] == want[M].split(), (layout, SHAPES[shape], M, dict(zip(KERNELS[layout], seen[M])))
