"""Return codes of the GEMM-layout entry points' host checks (csrc/capi.hip and the launchers behind it), without a GPU:
awq_gemm_forward, awq_gemm_forward_normed, awq_gemm_forward_ex, the grouped (MoE) forward and prefill entries with their _ex forms
and awq_dequantize_weights -- and the AUTO dispatch as awq_gemm_auto_kernel reports it.  The pointers are a small aligned HOST
buffer, so every call here has to return BEFORE any launch: each case carries at least one fault, an empty call, or a shape that
its path refuses on the host.  No case is a fully valid call, and AWQ_ERR_LAUNCH (-5) is never an expected code.

The expected codes and the dispatch table are literals.  They were fixed by running this file against the library as it stood before
these entry points were folded onto one checker, one argument fill and one dispatch; the two-fault cases pin the ORDER of the checks
where it differs between entry points (awq_gemm_forward_normed and _ex run their own checks before the shape rule and answer
aliasing residuals differently; the grouped forward refuses unknown flag bits before anything else; the plain grouped prefill
validates neither flag bits nor x_div)."""
import ctypes

import pytest

OK, BAD_SHAPE, BAD_ALIGNMENT, UNSUPPORTED, LAUNCH, NULL = 0, -1, -2, -3, -5, -6
NAIVE, VALU, MFMA_GEMV, TILED, REGB, SKINNY = 1, 2, 3, 4, 5, 6  # AWQ_GEMM_KERNEL_* in the low four flag bits
NLOG4, TWO_PASS, X_GATED = 4 << 4, 1 << 16, 1 << 18
GATHER, SCATTER = 1 << 19, 1 << 20  # AWQ_GROUPED_PREFILL_*
I32 = 1 << 31  # the first value past INT32_MAX

_buf = ctypes.create_string_buffer(256)
P = (ctypes.addressof(_buf) + 63) & ~63  # 16-byte aligned, never dereferenced
Q = P + 16                               # a second aligned address (what must not alias)

FWD, NORMED, EX = "awq_gemm_forward", "awq_gemm_forward_normed", "awq_gemm_forward_ex"
GFWD, GFWD_EX = "awq_grouped_gemm_forward", "awq_grouped_gemm_forward_ex"
GPRE, GPRE_EX = "awq_grouped_gemm_prefill", "awq_grouped_gemm_prefill_ex"
DEQ = "awq_dequantize_weights"
# the arguments of each entry point in ABI order (include/awq_hip.h), by role; awq_gemm_forward_ex: the fields of AwqGemmEx.
# pairs: the (token, expert) pairs of a grouped call (num_pairs / P); rows: block_rows; blocks: max_blocks
ENTRIES = {
    FWD: "x qw s qz bias y M K N g ws ws_bytes flags stream",
    NORMED: "x res_in res_out norm eps qw s qz bias y M K N g ws ws_bytes flags stream",
    EX: "struct_bytes flags x qw s qz bias y M K N g ws ws_bytes stream norm eps res_in res_out ssq_in tiles add_res ssq_out",
    GFWD: "x qw s qz y sorted eids npost pw pairs x_div rows blocks E K N g ws ws_bytes stream",
    GFWD_EX: "x qw s qz y sorted eids npost pw pairs x_div rows blocks E K N g ws ws_bytes flags stream",
    GPRE: "x qw s qz y seg pairs E K N g flags stream",
    GPRE_EX: "x qw s qz y seg rmap pw pairs x_div E K N g flags stream",
    DEQ: "qw s qz y K N g stream",
}
# a call that would be valid (and so is never made as it stands): one row of a 256 x 64 matrix in groups of 128 (the fused entries:
# with a norm weight); the grouped entries: two pairs over four experts, one block of 16 rows
VALID = dict(x=P, qw=P, s=P, qz=P, bias=None, y=P, M=1, K=256, N=64, g=128, ws=None, ws_bytes=0, flags=0, stream=None,
             norm=P, eps=1e-5, res_in=None, res_out=None, ssq_in=None, tiles=0, add_res=None, ssq_out=None, struct_bytes=None,
             sorted=P, eids=P, npost=P, pw=None, pairs=2, x_div=1, rows=16, blocks=1, E=4, seg=P, rmap=None)
PLAIN, FUSED = [FWD], [NORMED, EX]
FORWARD = PLAIN + FUSED
GROUPED_FWD, GROUPED_PRE = [GFWD, GFWD_EX], [GPRE, GPRE_EX]
MATMUL = FORWARD + GROUPED_FWD + GROUPED_PRE
OPERANDS = ("x", "qw", "s", "qz", "y")  # required and 16-byte aligned on every matmul entry


def is_empty(name, v):
    if name == DEQ:
        return v["K"] * v["N"] == 0
    if name in GROUPED_FWD:
        return v["pairs"] == 0 or v["blocks"] == 0 or v["N"] == 0
    return v["pairs" if name in GROUPED_PRE else "M"] == 0 or v["N"] == 0


def call(name, **faults):
    from autoawq_amd import _lib

    roles = ENTRIES[name].split()
    assert faults and set(faults) <= set(roles), (name, faults)
    v = {r: faults.get(r, VALID[r]) for r in roles}
    if name == EX:
        e = _lib.AwqGemmEx()
        e.struct_bytes = ctypes.sizeof(e) if v["struct_bytes"] is None else v["struct_bytes"]
        e.flags = v["flags"]
        e.x, e.qweight, e.scales, e.qzeros, e.bias, e.y = v["x"], v["qw"], v["s"], v["qz"], v["bias"], v["y"]
        e.M, e.K, e.N, e.group_size = v["M"], v["K"], v["N"], v["g"]
        e.workspace, e.workspace_bytes, e.stream = v["ws"], v["ws_bytes"], v["stream"]
        e.norm_weight, e.norm_eps, e.residual_in, e.residual_out = v["norm"], v["eps"], v["res_in"], v["res_out"]
        e.ssq_in, e.ssq_in_tiles, e.add_residual, e.ssq_out = v["ssq_in"], v["tiles"], v["add_res"], v["ssq_out"]
        rc = _lib.lib().awq_gemm_forward_ex(ctypes.byref(e))
    else:
        rc = getattr(_lib.lib(), name)(*[v[r] for r in roles])
    assert rc != LAUNCH, (name, faults)  # the call got as far as a launch: the case is wrong, not the library
    if rc == OK:  # only an empty call may succeed here: anything else ran a kernel on the host buffer
        assert is_empty(name, v), (name, faults)
    return rc


def _cases(names, among):
    return [(n, r) for n in names for r in ENTRIES[n].split() if r in among]


def test_the_table_names_every_entry_point():
    from autoawq_amd import _lib

    for name, roles in ENTRIES.items():
        if name == EX:
            assert len(roles.split()) == len(_lib.AwqGemmEx._fields_), name
        else:
            assert len(roles.split()) == len(_lib.SIGNATURES[name][1]), name


# ---- empty calls: OK before any pointer is looked at, but after the shape rule and the entry point's own range checks
def _nulls(name):
    return {r: None for r in ENTRIES[name].split() if r in OPERANDS + ("sorted", "eids", "npost", "seg", "ws")}


@pytest.mark.parametrize("name", [FWD, EX])
def test_empty_forward_is_ok(name):
    for empty in (dict(M=0), dict(N=0)):
        assert call(name, **empty) == OK
        assert call(name, **empty, **_nulls(name)) == OK
        assert call(name, **empty, x=P + 8, ws=P + 8) == OK
        assert call(name, **empty, flags=7) == OK
    assert call(name, M=0, K=-256) == BAD_SHAPE
    assert call(name, N=0, g=0) == BAD_SHAPE
    assert call(name, M=-1, N=0) == BAD_SHAPE
    assert call(name, M=0, K=0) == OK  # (K == 0 passes the rule)
    assert call(name, N=0, K=0) == OK


def test_empty_normed_forward_still_wants_its_norm_weight():
    assert call(NORMED, M=0) == OK
    assert call(NORMED, N=0) == OK
    assert call(NORMED, M=0, **_nulls(NORMED)) == OK
    assert call(NORMED, M=0, norm=None) == NULL
    assert call(NORMED, N=0, norm=P + 8) == BAD_ALIGNMENT
    assert call(NORMED, N=0, flags=X_GATED) == UNSUPPORTED
    assert call(NORMED, M=0, K=-256) == BAD_SHAPE


@pytest.mark.parametrize("name", GROUPED_FWD)
def test_empty_grouped_forward_is_ok(name):
    for empty in (dict(pairs=0), dict(blocks=0), dict(N=0)):
        assert call(name, **empty) == OK
        assert call(name, **empty, **_nulls(name)) == OK
        assert call(name, **empty, x=P + 8) == OK
        assert call(name, **empty, rows=12) == BAD_SHAPE
        assert call(name, **empty, E=0) == BAD_SHAPE
        assert call(name, **empty, g=0) == BAD_SHAPE


@pytest.mark.parametrize("name", GROUPED_PRE)
def test_empty_grouped_prefill_is_ok(name):
    for empty in (dict(pairs=0), dict(N=0)):
        assert call(name, **empty) == OK
        assert call(name, **empty, **_nulls(name)) == OK
        assert call(name, **empty, x=P + 8) == OK
        assert call(name, **empty, E=0) == BAD_SHAPE
        assert call(name, **empty, g=0) == BAD_SHAPE


def test_empty_matrix_dequantises_to_nothing():
    assert call(DEQ, K=0) == OK
    assert call(DEQ, N=0) == OK
    assert call(DEQ, K=0, qw=None, s=None, qz=None, y=None) == OK
    assert call(DEQ, N=0, y=P + 8) == OK
    assert call(DEQ, K=0, g=0) == BAD_SHAPE
    assert call(DEQ, N=0, g=96) == BAD_SHAPE


# ---- the shape rule, clause by clause
@pytest.mark.parametrize("name", [FWD, EX] + GROUPED_FWD + GROUPED_PRE + [DEQ])
def test_shape_rule(name):
    assert call(name, K=-256) == BAD_SHAPE
    assert call(name, N=-8) == BAD_SHAPE
    assert call(name, g=0) == BAD_SHAPE
    assert call(name, g=-128) == BAD_SHAPE
    assert call(name, N=68) == BAD_SHAPE           # N % 8
    assert call(name, g=96) == BAD_SHAPE           # K % group_size
    assert call(name, K=I32) == BAD_SHAPE
    assert call(name, N=I32) == BAD_SHAPE


@pytest.mark.parametrize("name", [FWD, EX])
def test_row_count_out_of_range(name):
    assert call(name, M=-1) == BAD_SHAPE
    assert call(name, M=I32) == BAD_SHAPE
    assert call(name, M=I32, x=None) == BAD_SHAPE


@pytest.mark.parametrize("name", GROUPED_FWD)
def test_grouped_forward_ranges(name):
    for rows in (0, 4, 12, 32, -8):
        assert call(name, rows=rows) == BAD_SHAPE
    assert call(name, pairs=-1) == BAD_SHAPE
    assert call(name, x_div=0) == BAD_SHAPE
    assert call(name, blocks=-1) == BAD_SHAPE
    assert call(name, E=0) == BAD_SHAPE
    assert call(name, E=0, x=None) == BAD_SHAPE


@pytest.mark.parametrize("name", GROUPED_PRE)
def test_grouped_prefill_ranges(name):
    assert call(name, pairs=-1) == BAD_SHAPE
    assert call(name, pairs=I32) == BAD_SHAPE
    assert call(name, E=0) == BAD_SHAPE
    assert call(name, E=4097) == BAD_SHAPE
    assert call(name, E=0, x=None) == BAD_SHAPE


# ---- required pointers, alignment
REQUIRED = _cases(MATMUL, OPERANDS + ("sorted", "eids", "npost", "seg")) + _cases([DEQ], ("qw", "s", "qz", "y")) + [(NORMED, "norm")]


@pytest.mark.parametrize("name,role", REQUIRED)
def test_required_pointer_null(name, role):
    assert call(name, **{role: None}) == NULL


ALIGNED = _cases(MATMUL, OPERANDS) + _cases(FORWARD, ("ws", "norm")) + [(DEQ, "s"), (DEQ, "y")]


@pytest.mark.parametrize("name,role", ALIGNED)
def test_misaligned_pointer(name, role):
    assert call(name, **{role: P + 8}) == BAD_ALIGNMENT


def test_fused_entries_own_pointers_misaligned():
    assert call(NORMED, res_in=P + 8, res_out=Q) == BAD_ALIGNMENT
    assert call(NORMED, res_in=Q, res_out=P + 8) == BAD_ALIGNMENT
    assert call(EX, res_in=P + 8, res_out=Q) == BAD_ALIGNMENT
    assert call(EX, res_in=Q, res_out=P + 8) == BAD_ALIGNMENT
    assert call(EX, add_res=P + 8) == BAD_ALIGNMENT
    assert call(EX, add_res=P + 8, norm=None) == BAD_ALIGNMENT


def test_unchecked_pointers_are_ignored():
    """misaligned together with a LATER fault: the later fault is what comes back"""
    assert call(FWD, bias=P + 8, flags=7) == UNSUPPORTED
    assert call(EX, bias=P + 8, M=5) == UNSUPPORTED
    assert call(EX, ssq_in=P + 8, tiles=1, M=5) == UNSUPPORTED
    assert call(EX, ssq_out=P + 8, M=5) == UNSUPPORTED
    for name in GROUPED_FWD:
        assert call(name, sorted=P + 8, eids=P + 8, npost=P + 8, pw=P + 8, ws=P + 8, blocks=65536) == UNSUPPORTED
    assert call(GPRE, seg=P + 8, g=32) == UNSUPPORTED
    assert call(GPRE_EX, seg=P + 8, rmap=P + 8, pw=P + 8, g=32) == UNSUPPORTED


# ---- the kernel field and the shapes a path refuses on the host
def test_unknown_kernel_number():
    for kern in range(7, 16):
        assert call(FWD, flags=kern) == UNSUPPORTED
        assert call(FWD, flags=kern, M=300) == UNSUPPORTED
    assert call(FWD, flags=7, x=None) == NULL
    assert call(FWD, flags=7, s=P + 8) == BAD_ALIGNMENT
    assert call(FWD, flags=7, ws=P + 8) == BAD_ALIGNMENT
    assert call(FWD, flags=7, g=96) == BAD_SHAPE


def test_explicit_kernel_that_refuses_the_shape():
    """no fallback for a kernel the caller names"""
    for M in (17, 64, 300):
        assert call(FWD, flags=MFMA_GEMV, M=M) == UNSUPPORTED
    assert call(FWD, flags=MFMA_GEMV, N=72) == UNSUPPORTED         # N % 32
    assert call(FWD, flags=MFMA_GEMV | 3 << 4) == UNSUPPORTED      # three words per lane
    assert call(FWD, flags=MFMA_GEMV | 4 << 4, M=9) == UNSUPPORTED  # four words per lane: eight rows
    assert call(FWD, flags=VALU, M=5) == UNSUPPORTED
    assert call(FWD, flags=VALU, N=72) == UNSUPPORTED
    assert call(FWD, flags=VALU | 5 << 4) == UNSUPPORTED
    assert call(FWD, flags=TILED, K=96, g=32) == UNSUPPORTED       # K % 64
    assert call(FWD, flags=TILED | 2 << 4, K=96, g=32) == UNSUPPORTED
    assert call(FWD, flags=REGB, g=32) == UNSUPPORTED
    assert call(FWD, flags=REGB | 1 << 4, M=300, g=32) == UNSUPPORTED
    assert call(FWD, flags=SKINNY) == UNSUPPORTED                  # nine rows at least
    assert call(FWD, flags=SKINNY, M=65) == UNSUPPORTED
    assert call(FWD, flags=SKINNY, M=32, g=32) == UNSUPPORTED      # (named: not replaced by the tiled kernel)


@pytest.mark.parametrize("name", FORWARD)
def test_offsets_past_32_bits(name):
    assert call(name, K=65536, N=65536) == UNSUPPORTED
    assert call(name, K=65536, N=65536, qw=None) == NULL
    assert call(name, K=65536, N=65536, y=P + 8) == BAD_ALIGNMENT
    assert call(name, K=65536, N=65536, ws=P + 8) == BAD_ALIGNMENT
    assert call(name, K=65536, N=65536, flags=7) == UNSUPPORTED
    assert call(name, K=65536, N=65536, M=0) == OK


def test_gated_activations_are_the_decode_kernels():
    for M in (17, 64, 300):
        assert call(FWD, flags=X_GATED, M=M) == UNSUPPORTED
    assert call(FWD, flags=X_GATED, N=72) == UNSUPPORTED
    assert call(FWD, flags=X_GATED, g=48, K=96) == UNSUPPORTED
    for kern in (NAIVE, VALU, TILED, REGB, SKINNY, 7):
        assert call(FWD, flags=X_GATED | kern) == UNSUPPORTED
        assert call(FWD, flags=X_GATED | kern, M=9) == UNSUPPORTED
    assert call(FWD, flags=X_GATED | TILED, x=None) == NULL
    assert call(FWD, flags=X_GATED | TILED, ws=P + 8) == BAD_ALIGNMENT
    assert call(FWD, flags=X_GATED, M=17, K=65536, N=65536) == UNSUPPORTED


@pytest.mark.parametrize("name", FUSED)
def test_fused_forward_refusals(name):
    for M in (5, 16, 17, 300):
        assert call(name, M=M) == UNSUPPORTED
    assert call(name, flags=X_GATED) == UNSUPPORTED                # with a norm weight
    assert call(name, flags=TWO_PASS) == UNSUPPORTED
    assert call(name, flags=NLOG4) == UNSUPPORTED
    assert call(name, N=72) == UNSUPPORTED                         # a shape the decode kernel refuses
    for kern in (NAIVE, VALU, TILED, REGB, SKINNY, 7):
        assert call(name, flags=kern) == UNSUPPORTED
        assert call(name, flags=kern, M=4) == UNSUPPORTED
    assert call(name, flags=MFMA_GEMV | 3 << 4) == UNSUPPORTED     # the decode kernel, named, with a width it does not have


def test_ex_without_a_norm_is_still_the_decode_kernel_alone():
    """an _ex call with only an epilogue (or nothing at all) sets no gated mode, and is restricted all the same"""
    for extras in (dict(add_res=Q), dict(ssq_out=P), dict(bias=P)):
        assert call(EX, norm=None, M=5, **extras) == UNSUPPORTED
        assert call(EX, norm=None, M=17, **extras) == UNSUPPORTED
        assert call(EX, norm=None, flags=TILED, **extras) == UNSUPPORTED
        assert call(EX, norm=None, flags=TWO_PASS, **extras) == UNSUPPORTED
        assert call(EX, norm=None, flags=NLOG4, **extras) == UNSUPPORTED
        assert call(EX, norm=None, N=72, **extras) == UNSUPPORTED
    assert call(EX, norm=None, flags=X_GATED, M=5) == UNSUPPORTED
    assert call(EX, norm=None, flags=X_GATED | SKINNY) == UNSUPPORTED


# ---- awq_gemm_forward_normed: its own checks come before the shape rule, in this order
def test_normed_own_checks_and_their_order():
    assert call(NORMED, norm=None) == NULL
    assert call(NORMED, res_in=P) == NULL                          # one residual without the other
    assert call(NORMED, res_out=P) == NULL
    assert call(NORMED, res_in=Q, res_out=Q) == BAD_ALIGNMENT      # aliasing residuals
    assert call(NORMED, M=5) == UNSUPPORTED
    assert call(NORMED, flags=X_GATED) == UNSUPPORTED
    # each before the one after it
    assert call(NORMED, norm=None, res_in=Q, res_out=Q) == NULL
    assert call(NORMED, norm=None, M=5) == NULL
    assert call(NORMED, res_in=P, norm=P + 8) == NULL
    assert call(NORMED, res_in=P, M=5) == NULL
    assert call(NORMED, res_in=Q, res_out=Q, M=5) == BAD_ALIGNMENT
    assert call(NORMED, norm=P + 8, M=5) == BAD_ALIGNMENT
    assert call(NORMED, res_in=P + 8, res_out=Q, flags=X_GATED) == BAD_ALIGNMENT
    # all before the shape rule, the empty call and the operands
    assert call(NORMED, norm=None, K=-256) == NULL
    assert call(NORMED, res_in=Q, res_out=Q, g=96) == BAD_ALIGNMENT
    assert call(NORMED, M=5, K=-256) == UNSUPPORTED
    assert call(NORMED, M=5, x=None) == UNSUPPORTED
    assert call(NORMED, M=I32) == UNSUPPORTED
    assert call(NORMED, flags=X_GATED, N=0) == UNSUPPORTED
    assert call(NORMED, M=-1) == BAD_SHAPE
    assert call(NORMED, M=4, K=-256) == BAD_SHAPE
    assert call(NORMED, M=4, x=None) == NULL
    assert call(NORMED, M=4, y=P + 8) == BAD_ALIGNMENT


# ---- awq_gemm_forward_ex
def test_ex_struct():
    from autoawq_amd import _lib

    assert _lib.lib().awq_gemm_forward_ex(None) == NULL            # (awq_gemv_forward_ex: BAD_SHAPE)
    size = ctypes.sizeof(_lib.AwqGemmEx)
    assert call(EX, struct_bytes=size - 8) == BAD_SHAPE
    assert call(EX, struct_bytes=size + 8) == BAD_SHAPE
    assert call(EX, struct_bytes=0, M=0) == BAD_SHAPE
    assert call(EX, struct_bytes=0, res_in=P) == BAD_SHAPE


def test_ex_own_checks_and_their_order():
    assert call(EX, res_in=P) == NULL
    assert call(EX, res_out=P) == NULL
    assert call(EX, res_in=Q, res_out=Q) == BAD_SHAPE              # aliasing residuals (_normed: BAD_ALIGNMENT)
    assert call(EX, res_in=P, res_out=Q, norm=None) == BAD_SHAPE   # a residual stream wants the norm
    assert call(EX, ssq_in=P, tiles=1, norm=None) == BAD_SHAPE
    assert call(EX, ssq_in=P, tiles=1, res_in=P, res_out=Q) == BAD_SHAPE
    assert call(EX, ssq_in=P, tiles=0) == BAD_SHAPE
    assert call(EX, ssq_in=P, tiles=65) == BAD_SHAPE
    assert call(EX, add_res=P) == BAD_SHAPE                        # the output itself
    # before the shape rule, the empty call and the operands
    assert call(EX, res_in=P, K=-256) == NULL
    assert call(EX, res_in=P, M=0) == NULL
    assert call(EX, add_res=P + 8, K=-256) == BAD_ALIGNMENT
    assert call(EX, norm=P + 8, M=0) == BAD_ALIGNMENT
    assert call(EX, add_res=P + 8, x=None) == BAD_ALIGNMENT
    assert call(EX, res_in=Q, res_out=Q, x=None) == BAD_SHAPE
    assert call(EX, res_in=P, add_res=P) == NULL
    assert call(EX, add_res=P, norm=P + 8) == BAD_SHAPE
    # the restriction to small batches comes AFTER the shape rule and the operands here (_normed: before)
    assert call(EX, M=5, K=-256) == BAD_SHAPE
    assert call(EX, M=5, x=None) == NULL
    assert call(EX, M=5, y=P + 8) == BAD_ALIGNMENT
    assert call(EX, M=5, ws=P + 8) == BAD_ALIGNMENT
    assert call(EX, M=5, N=0) == OK


# ---- the grouped (MoE) entries
def test_grouped_forward_flags_come_first():
    for flags in (1, TILED, TWO_PASS, X_GATED | 1, GATHER):
        assert call(GFWD_EX, flags=flags) == UNSUPPORTED
        assert call(GFWD_EX, flags=flags, K=-256) == UNSUPPORTED
        assert call(GFWD_EX, flags=flags, rows=12) == UNSUPPORTED
        assert call(GFWD_EX, flags=flags, pairs=0) == UNSUPPORTED
        assert call(GFWD_EX, flags=flags, x=None) == UNSUPPORTED
    assert call(GFWD_EX, flags=X_GATED, K=-256) == BAD_SHAPE
    assert call(GFWD_EX, flags=X_GATED, pairs=0) == OK
    assert call(GFWD_EX, flags=X_GATED, x=None) == NULL


@pytest.mark.parametrize("name", GROUPED_FWD)
def test_grouped_forward_limits_come_after_the_pointers(name):
    assert call(name, blocks=65536) == UNSUPPORTED                 # token blocks ride in the grid's z
    assert call(name, N=72) == UNSUPPORTED                         # a shape the decode kernel refuses
    assert call(name, g=48, K=96) == UNSUPPORTED
    assert call(name, K=65536, N=65536) == UNSUPPORTED
    assert call(name, K=65536, N=65536, E=1024) == UNSUPPORTED     # the whole stack past 2^40 bytes
    assert call(name, blocks=65536, x=None) == NULL
    assert call(name, blocks=65536, npost=None) == NULL
    assert call(name, K=65536, N=65536, qw=P + 8) == BAD_ALIGNMENT
    assert call(name, N=72, rows=12) == BAD_SHAPE
    assert call(name, rows=12, g=96) == BAD_SHAPE


def test_grouped_prefill_flags_and_x_div():
    """the plain entry validates neither; _ex validates both, before the empty call"""
    for flags in (1, 7, TWO_PASS, X_GATED, 1 << 25):
        assert call(GPRE_EX, flags=flags) == BAD_SHAPE
        assert call(GPRE_EX, flags=flags, pairs=0) == BAD_SHAPE
        assert call(GPRE_EX, flags=flags, x=None) == BAD_SHAPE
        assert call(GPRE, flags=flags, pairs=0) == OK
        assert call(GPRE, flags=flags, x=None) == NULL
        assert call(GPRE, flags=flags, g=32) == UNSUPPORTED
    assert call(GPRE_EX, x_div=0) == BAD_SHAPE
    assert call(GPRE_EX, x_div=0, pairs=0) == BAD_SHAPE
    assert call(GPRE_EX, flags=0xF0, pairs=0) == OK                # the tile-height field
    assert call(GPRE_EX, flags=0xF0, g=32) == UNSUPPORTED
    assert call(GPRE, flags=3 << 4, g=32) == UNSUPPORTED


def test_grouped_prefill_row_map():
    for extras in (dict(flags=GATHER), dict(flags=SCATTER), dict(pw=P), dict(flags=GATHER | SCATTER, pw=P)):
        assert call(GPRE_EX, **extras) == NULL                     # (rmap is NULL in the valid call)
        assert call(GPRE_EX, x=P + 8, **extras) == NULL            # before the alignment
        assert call(GPRE_EX, pairs=0, **extras) == OK              # after the empty call
        assert call(GPRE_EX, rmap=P, g=32, **extras) == UNSUPPORTED
    assert call(GPRE_EX, rmap=P, x=P + 8) == BAD_ALIGNMENT


@pytest.mark.parametrize("name", GROUPED_PRE)
def test_grouped_prefill_shapes_the_kernel_refuses(name):
    assert call(name, g=32) == UNSUPPORTED                         # groups of 64 rows at least
    assert call(name, K=96, g=96) == UNSUPPORTED                   # K % 64
    assert call(name, K=65536, N=64, g=128) == UNSUPPORTED         # K < 65536
    assert call(name, g=32, x=None) == NULL
    assert call(name, g=32, seg=None) == NULL
    assert call(name, g=32, s=P + 8) == BAD_ALIGNMENT
    assert call(name, g=32, E=4097) == BAD_SHAPE


# ---- two faults at once: which check comes first
@pytest.mark.parametrize("name", [FWD, EX] + GROUPED_FWD + GROUPED_PRE)
def test_order_shape_null_alignment(name):
    assert call(name, x=None, K=-256) == BAD_SHAPE
    assert call(name, x=P + 8, g=96) == BAD_SHAPE
    assert call(name, x=P + 8, qw=None) == NULL
    assert call(name, s=None, x=P + 8) == NULL
    assert call(name, y=None, qw=P + 8) == NULL
    assert call(name, x=None, N=0) == OK


def test_order_dequantise():
    assert call(DEQ, y=P + 8, qw=None) == NULL
    assert call(DEQ, s=P + 8, y=None) == NULL
    assert call(DEQ, y=P + 8, g=96) == BAD_SHAPE
    assert call(DEQ, y=None, N=68) == BAD_SHAPE
    assert call(DEQ, y=P + 8, N=0) == OK


# ---- the AUTO dispatch, as awq_gemm_auto_kernel reports it (host only)
AUTO_ROWS = [1, 4, 8, 9, 12, 16, 17, 32, 33, 64, 65, 128, 512, 768, 2048, 16384]
# (K, N, group_size): the five BASELINE shapes; a shape only the naive kernel decodes; a tall one (K = 8192: the decode kernel keeps
# 9 .. 16 rows); one just past the width the batched kernel's reducers cover at M > 32; groups of 32 rows (no register-decoded kernel)
AUTO_TABLE = {
    (4096, 4096, 128): "3 3 3 6 6 6 6 6 6 6 4 4 4 4 5 5",
    (4096, 11008, 128): "3 3 3 6 6 6 6 6 6 6 4 4 4 5 5 5",
    (11008, 4096, 128): "3 3 3 3 3 3 6 6 6 6 4 4 4 4 5 5",
    (4096, 12288, 128): "3 3 3 6 6 6 6 6 6 6 4 4 4 5 5 5",
    (4096, 22016, 128): "3 3 3 3 3 3 6 6 4 4 4 4 5 5 5 5",
    (256, 40, 128): "1 1 1 6 6 6 6 6 6 6 4 4 4 4 4 4",
    (8192, 4096, 128): "3 3 3 3 3 3 6 6 6 6 4 4 4 4 5 5",
    (4096, 16640, 128): "3 3 3 3 3 3 6 6 4 4 4 4 5 5 5 5",
    (4096, 4096, 32): "3 3 3 3 3 3 4 4 4 4 4 4 4 4 4 4",
}


def test_auto_dispatch_table():
    from autoawq_amd import _lib

    L = _lib.lib()
    seen = set()
    for (K, N, g), want in AUTO_TABLE.items():
        got = [L.awq_gemm_auto_kernel(M, K, N, g) for M in AUTO_ROWS]
        print((K, N, g), " ".join(map(str, got)))
        assert got == [int(k) for k in want.split()], (K, N, g, dict(zip(AUTO_ROWS, got)))
        seen |= set(got)
    assert seen == {NAIVE, MFMA_GEMV, TILED, REGB, SKINNY}  # every kernel AUTO can return (the VALU kernel is explicit only)


def test_auto_dispatch_invalid_shapes():
    from autoawq_amd import _lib

    q = _lib.lib().awq_gemm_auto_kernel
    for M, K, N, g in [(0, 4096, 4096, 128), (-1, 4096, 4096, 128), (I32, 4096, 4096, 128), (1, 0, 4096, 128), (1, 4096, 0, 128),
                       (1, 4096, 4100, 128), (1, 4096, 4096, 0), (1, 4096, 4096, 96), (1, I32, 4096, 128), (1, 4096, I32, 128)]:
        assert q(M, K, N, g) == -1, (M, K, N, g)
