"""Return codes of the GEMV- and GEMVFast-layout entry points' host checks (csrc/capi.hip and the launchers behind it), without a
GPU: awq_gemv_forward, awq_gemv_forward_ex, awq_grouped_gemv_forward, awq_gemv_fast_forward, awq_gemv_fast_prefill and the two
dequantisers.  The pointers are a small aligned HOST buffer, so every call here has to return BEFORE any launch: each case carries
at least one fault, an empty M / N, or a shape that every kernel of its path refuses on the host.  No case is a fully valid call,
and AWQ_ERR_LAUNCH (-5) is never an expected code.

The expected codes are literals.  They were fixed by running this file against the library as it stood before the entry points
were folded onto one argument struct, one checker and one dispatch per layout; the two-fault cases pin the ORDER of the checks
where it differs between entry points (awq_gemv_forward_ex refuses M != 1 only after the pointer and alignment checks, the
grouped entry its limits after them; awq_gemv_forward looks at y's alignment for the PREFILL kernel alone)."""
import ctypes

import pytest

OK, BAD_SHAPE, BAD_ALIGNMENT, UNSUPPORTED, LAUNCH, NULL = 0, -1, -2, -3, -5, -6
TILE16, ROWS, LDS, PREFILL, BATCH = 1, 2, 3, 4, 5  # AWQ_GEMV_KERNEL_* in the low four flag bits
PAIRS = 1  # AWQ_GEMV_EX_SILU_PAIRS
I32 = 1 << 31  # the first value past INT32_MAX

_buf = ctypes.create_string_buffer(256)
P = (ctypes.addressof(_buf) + 63) & ~63  # 16-byte aligned, never dereferenced

FWD, EX, GROUPED = "awq_gemv_forward", "awq_gemv_forward_ex", "awq_grouped_gemv_forward"
FAST, FAST_PREFILL = "awq_gemv_fast_forward", "awq_gemv_fast_prefill"
DEQ, DEQ_FAST = "awq_dequantize_weights_gemv", "awq_dequantize_weights_gemv_fast"
# the arguments of each entry point in ABI order (include/awq_hip.h), by role; awq_gemv_forward_ex: the fields call() puts into
# its AwqGemvEx.  W: the layout's width (zeros_width on GEMV, group_rows on GEMVFast)
ENTRIES = {
    FWD: "x qw s qz y M K N g W flags stream",
    EX: "x qw s qz y M K N g W flags stream norm res struct_bytes",
    GROUPED: "x qw s qz y pe pw pairs x_div E first K N g W flags parts stream",
    FAST: "x qw s qz y M K N g W flags stream",
    FAST_PREFILL: "x qw s qz y tmp M K N g W flags stream",
    DEQ: "qw s qz y K N g W stream",
    DEQ_FAST: "qw s qz y K N g stream",
}
# a call that would be valid (and so is never made as it stands): one row of a 256 x 64 matrix in groups of 128; the grouped entry:
# two (token, expert) pairs over four experts
VALID = dict(x=P, qw=P, s=P, qz=P, y=P, tmp=P, pe=P, pw=None, norm=None, res=None, M=1, K=256, N=64, g=128, W=8, flags=0, stream=None,
             pairs=2, x_div=1, E=4, first=0, parts=0, struct_bytes=None)
MATMUL = [FWD, EX, GROUPED, FAST, FAST_PREFILL]
GEMV = [FWD, EX, GROUPED]          # the GEMV layout's three
FASTS = [FAST, FAST_PREFILL]
ROWS_NAME = {GROUPED: "pairs"}     # the role that counts the rows of the call


def call(name, **faults):
    from autoawq_amd import _lib

    roles = ENTRIES[name].split()
    assert faults and set(faults) <= set(roles), (name, faults)
    v = {r: faults.get(r, VALID[r]) for r in roles}
    if name == EX:
        e = _lib.AwqGemvEx()
        e.struct_bytes = ctypes.sizeof(e) if v["struct_bytes"] is None else v["struct_bytes"]
        e.flags = v["flags"]
        e.x, e.qweight, e.scales, e.qzeros, e.y = v["x"], v["qw"], v["s"], v["qz"], v["y"]
        e.M, e.K, e.N, e.group_size, e.zeros_width = v["M"], v["K"], v["N"], v["g"], v["W"]
        e.stream, e.norm_weight, e.norm_eps, e.add_residual = v["stream"], v["norm"], 1e-5, v["res"]
        rc = _lib.lib().awq_gemv_forward_ex(ctypes.byref(e))
    else:
        rc = getattr(_lib.lib(), name)(*[v[r] for r in roles])
    assert rc != LAUNCH, (name, faults)  # the call got as far as a launch: the case is wrong, not the library
    if rc == OK:  # only an empty call may succeed here: anything else ran a kernel on the host buffer
        empty = v["K"] * v["N"] == 0 if name in (DEQ, DEQ_FAST) else v[ROWS_NAME.get(name, "M")] == 0 or v["N"] == 0
        assert empty, (name, faults)
    return rc


def _cases(names, among):
    return [(n, r) for n in names for r in ENTRIES[n].split() if r in among]


def test_the_table_names_every_entry_point():
    from autoawq_amd import _lib

    for name, roles in ENTRIES.items():
        if name == EX:
            assert len(roles.split()) == len(_lib.AwqGemvEx._fields_) - 1, name  # (norm_eps is not a role)
        else:
            assert len(roles.split()) == len(_lib.SIGNATURES[name][1]), name


# ---- empty calls: OK before any pointer is looked at, but after the shape rule
@pytest.mark.parametrize("name", MATMUL)
def test_empty_call_is_ok(name):
    rows = ROWS_NAME.get(name, "M")
    nulls = {r: None for r in ENTRIES[name].split() if r in ("x", "qw", "s", "qz", "y", "tmp", "pe")}
    assert call(name, **{rows: 0}) == OK
    assert call(name, N=0) == OK
    assert call(name, **{rows: 0}, **nulls) == OK
    assert call(name, N=0, **nulls) == OK
    assert call(name, **{rows: 0}, x=P + 8) == OK
    assert call(name, **{rows: 0}, K=0) == BAD_SHAPE
    assert call(name, N=0, g=0) == BAD_SHAPE
    assert call(name, **{rows: 0}, W=0) == BAD_SHAPE


@pytest.mark.parametrize("name", [DEQ, DEQ_FAST])
def test_empty_matrix_dequantises_to_nothing(name):
    assert call(name, K=0) == OK
    assert call(name, N=0) == OK
    assert call(name, K=0, qw=None, s=None, qz=None, y=None) == OK
    assert call(name, N=0, y=None) == OK
    assert call(name, K=0, g=0) == BAD_SHAPE
    assert call(name, K=0, g=96) == OK  # (K == 0 is a multiple of nothing in particular: the group rule is skipped)


# ---- the shape rule, clause by clause
@pytest.mark.parametrize("name", GEMV)
def test_gemv_shape_rule(name):
    assert call(name, K=0) == BAD_SHAPE
    assert call(name, K=-256) == BAD_SHAPE
    assert call(name, N=-8) == BAD_SHAPE
    assert call(name, g=0) == BAD_SHAPE
    assert call(name, g=-128) == BAD_SHAPE
    assert call(name, g=96) == BAD_SHAPE           # K % group_size
    assert call(name, K=12, g=12) == BAD_SHAPE     # K % 8 alone
    assert call(name, W=0) == BAD_SHAPE
    assert call(name, W=-1) == BAD_SHAPE
    assert call(name, g=8, W=3) == BAD_SHAPE       # 32 groups need four words of zeros
    assert call(name, K=I32, W=1 << 21) == BAD_SHAPE
    assert call(name, N=I32) == BAD_SHAPE


@pytest.mark.parametrize("name", [FWD, EX, FAST, FAST_PREFILL])
def test_row_count_out_of_range(name):
    assert call(name, M=-1) == BAD_SHAPE
    assert call(name, M=I32) == BAD_SHAPE
    assert call(name, M=-1, N=0) == BAD_SHAPE


@pytest.mark.parametrize("name", FASTS)
def test_gemv_fast_shape_rule(name):
    assert call(name, K=0) == BAD_SHAPE
    assert call(name, K=-256) == BAD_SHAPE
    assert call(name, N=-8) == BAD_SHAPE
    assert call(name, g=0) == BAD_SHAPE
    assert call(name, g=-128) == BAD_SHAPE
    assert call(name, g=96) == BAD_SHAPE           # K % group_size
    assert call(name, N=66) == BAD_SHAPE           # N % 4
    assert call(name, K=96, g=32) == BAD_SHAPE     # K % 64 alone
    assert call(name, W=1) == BAD_SHAPE            # two groups need two rows of scales
    assert call(name, W=0) == BAD_SHAPE
    assert call(name, K=I32, W=1 << 24) == BAD_SHAPE
    assert call(name, N=I32) == BAD_SHAPE


def test_dequantise_shape_rules():
    """Looser than the forward entries': no range, no width."""
    for name in (DEQ, DEQ_FAST):
        assert call(name, K=-256) == BAD_SHAPE
        assert call(name, N=-8) == BAD_SHAPE
        assert call(name, g=0) == BAD_SHAPE
        assert call(name, g=-128) == BAD_SHAPE
        assert call(name, g=96) == BAD_SHAPE
    assert call(DEQ, K=12, g=12) == BAD_SHAPE      # K % 8
    assert call(DEQ, K=240, g=20) == BAD_SHAPE     # group_size % 8
    assert call(DEQ, W=0, qw=None) == NULL         # the width is not looked at
    assert call(DEQ_FAST, K=96, g=32) == BAD_SHAPE  # K % 64
    assert call(DEQ_FAST, N=66) == BAD_SHAPE        # N % 4


# ---- required pointers
@pytest.mark.parametrize("name,role", _cases(ENTRIES, ("x", "qw", "s", "qz", "y", "tmp", "pe")))
def test_required_pointer_null(name, role):
    assert call(name, **{role: None}) == NULL


# ---- alignment: x, qweight and scales everywhere; qzeros on GEMVFast alone; y and the temporary where the prefill GEMM writes them;
# the norm weight of _ex; the dequantised matrix on the GEMV layout
CHECKED = _cases(MATMUL, ("x", "qw", "s")) + _cases(FASTS, ("qz",)) + [(FAST_PREFILL, "y"), (FAST_PREFILL, "tmp"), (EX, "norm"), (DEQ, "y")]


@pytest.mark.parametrize("name,role", CHECKED)
def test_misaligned_pointer(name, role):
    assert call(name, **{role: P + 8}) == BAD_ALIGNMENT


def test_output_alignment_only_for_the_prefill_kernel():
    assert call(FWD, y=P + 8, flags=PREFILL) == BAD_ALIGNMENT
    assert call(FWD, y=P + 8, flags=PREFILL, x=None) == NULL
    assert call(FWD, y=P + 8, flags=PREFILL, M=0) == OK
    for kern in (0, TILE16, ROWS, LDS, BATCH, 7):
        assert call(FWD, y=P + 8, flags=kern, K=64, g=64) == UNSUPPORTED  # (no decode kernel takes K = 64)


def test_unchecked_pointers_are_ignored():
    """misaligned together with a LATER fault: the later fault is what comes back"""
    assert call(FWD, qz=P + 8, M=17, flags=TILE16) == UNSUPPORTED
    assert call(FWD, y=P + 8, M=17, flags=TILE16) == UNSUPPORTED
    assert call(FWD, qz=P + 8, flags=PREFILL, g=32) == UNSUPPORTED
    assert call(EX, qz=P + 8, M=2) == UNSUPPORTED
    assert call(EX, y=P + 8, M=2) == UNSUPPORTED
    assert call(EX, res=P + 8, M=2) == UNSUPPORTED
    assert call(GROUPED, qz=P + 8, pairs=8192) == UNSUPPORTED
    assert call(GROUPED, y=P + 8, pairs=8192) == UNSUPPORTED
    assert call(GROUPED, pe=P + 8, pw=P + 8, pairs=8192) == UNSUPPORTED
    assert call(FAST, y=P + 8, M=17, flags=1) == UNSUPPORTED


# ---- awq_gemv_forward_ex
def test_ex_struct_and_flags():
    from autoawq_amd import _lib

    assert _lib.lib().awq_gemv_forward_ex(None) == BAD_SHAPE
    size = ctypes.sizeof(_lib.AwqGemvEx)
    assert call(EX, struct_bytes=size - 8) == BAD_SHAPE
    assert call(EX, struct_bytes=size + 8) == BAD_SHAPE
    assert call(EX, struct_bytes=0, M=0) == BAD_SHAPE
    assert call(EX, flags=2) == BAD_SHAPE
    assert call(EX, flags=PAIRS | 4) == BAD_SHAPE
    assert call(EX, flags=2, M=0) == BAD_SHAPE


def test_ex_pairs():
    assert call(EX, flags=PAIRS, res=P) == BAD_SHAPE
    assert call(EX, flags=PAIRS, N=63) == BAD_SHAPE
    assert call(EX, flags=PAIRS, res=P, M=0) == BAD_SHAPE  # before the empty call
    assert call(EX, flags=PAIRS, N=63, x=None) == BAD_SHAPE
    assert call(EX, flags=PAIRS, M=0) == OK


def test_ex_takes_one_row():
    for M in (2, 4, 17):
        assert call(EX, M=M) == UNSUPPORTED
    assert call(EX, M=2, x=None) == NULL            # only after the pointer ...
    assert call(EX, M=2, s=P + 8) == BAD_ALIGNMENT  # ... and alignment checks
    assert call(EX, M=2, norm=P + 8) == BAD_ALIGNMENT
    assert call(EX, M=2, K=0) == BAD_SHAPE
    assert call(EX, g=64) == UNSUPPORTED            # one row of a shape the row-streaming kernel refuses
    assert call(EX, K=64, g=64) == UNSUPPORTED


# ---- awq_grouped_gemv_forward
def test_grouped_shape():
    assert call(GROUPED, first=-1) == BAD_SHAPE
    assert call(GROUPED, first=I32) == BAD_SHAPE
    assert call(GROUPED, first=-1, pairs=0) == BAD_SHAPE
    assert call(GROUPED, pairs=-1) == BAD_SHAPE
    assert call(GROUPED, E=0) == BAD_SHAPE
    assert call(GROUPED, E=I32) == BAD_SHAPE
    assert call(GROUPED, x_div=0) == BAD_SHAPE
    assert call(GROUPED, parts=-1) == BAD_SHAPE
    assert call(GROUPED, flags=2) == BAD_SHAPE
    assert call(GROUPED, flags=PAIRS, pw=P) == BAD_SHAPE
    assert call(GROUPED, flags=PAIRS, N=63) == BAD_SHAPE
    assert call(GROUPED, flags=PAIRS, pw=P, pairs=0) == BAD_SHAPE
    assert call(GROUPED, flags=PAIRS, pairs=0) == OK


def test_grouped_limits_come_after_the_pointers():
    assert call(GROUPED, pairs=8192) == UNSUPPORTED
    assert call(GROUPED, parts=65536) == UNSUPPORTED
    assert call(GROUPED, x_div=3) == UNSUPPORTED                # more tokens than pairs
    assert call(GROUPED, K=8, N=1, g=8, W=1) == UNSUPPORTED     # an expert's words are 4 bytes: the stack's second expert is misaligned
    assert call(GROUPED, pairs=8192, x=None) == NULL
    assert call(GROUPED, pairs=8192, pe=None) == NULL
    assert call(GROUPED, parts=65536, qw=P + 8) == BAD_ALIGNMENT
    assert call(GROUPED, x_div=3, s=P + 8) == BAD_ALIGNMENT
    assert call(GROUPED, pairs=8192, N=I32) == BAD_SHAPE
    assert call(GROUPED, pairs=I32) == UNSUPPORTED              # (the pair count has no range of its own)
    assert call(GROUPED, pairs=I32, x_div=I32, parts=I32) == UNSUPPORTED
    assert call(GROUPED, g=64) == UNSUPPORTED                   # a shape the row-streaming kernel refuses
    assert call(GROUPED, K=64, g=64) == UNSUPPORTED


# ---- the kernel field
def test_gemv_more_rows_than_a_decode_kernel_takes():
    for kern in (TILE16, ROWS, LDS, 7):
        assert call(FWD, M=17, flags=kern) == UNSUPPORTED
        assert call(FWD, M=300, flags=kern) == UNSUPPORTED
        assert call(FWD, M=17, flags=kern, x=None) == NULL
        assert call(FWD, M=17, flags=kern, qw=P + 8) == BAD_ALIGNMENT


def test_gemv_explicit_kernel_that_refuses_the_shape():
    """no fallback: ROWS and LDS want groups of 128 (LDS also two rows), BATCH groups of 128"""
    assert call(FWD, flags=ROWS, g=64) == UNSUPPORTED
    assert call(FWD, flags=ROWS, M=5) == UNSUPPORTED
    assert call(FWD, flags=LDS, g=64, M=2) == UNSUPPORTED
    assert call(FWD, flags=LDS) == UNSUPPORTED
    assert call(FWD, flags=BATCH, g=64) == UNSUPPORTED
    assert call(FWD, flags=BATCH, g=64, M=200) == UNSUPPORTED
    assert call(FWD, flags=BATCH, K=64, g=64) == UNSUPPORTED
    assert call(FWD, flags=PREFILL, g=32) == UNSUPPORTED
    assert call(FWD, flags=PREFILL, g=32, M=300) == UNSUPPORTED


@pytest.mark.parametrize("M", [1, 2, 4, 5, 16, 17, 300])
def test_gemv_shape_no_decode_kernel_takes(M):
    for kern in (0, TILE16, ROWS, LDS, BATCH, 7):
        assert call(FWD, M=M, flags=kern, K=64, g=64) == UNSUPPORTED


def test_gemv_fast_kernel_field():
    for kern in (1, 2, 7):  # any number but 0 and BATCH: the 16-row kernel
        assert call(FAST, M=17, flags=kern) == UNSUPPORTED
        assert call(FAST, M=300, flags=kern) == UNSUPPORTED
        assert call(FAST, M=17, flags=kern, qz=None) == NULL
        assert call(FAST, M=17, flags=kern, qz=P + 8) == BAD_ALIGNMENT
    assert call(FAST, flags=BATCH, g=64) == UNSUPPORTED
    assert call(FAST, flags=BATCH, g=64, M=300) == UNSUPPORTED
    assert call(FAST, g=64, M=17) == UNSUPPORTED    # AUTO: the batched kernel refuses the groups, the 16-row kernel the rows
    assert call(FAST, N=68) == UNSUPPORTED          # N % 16: neither kernel
    assert call(FAST, N=68, M=17, flags=BATCH) == UNSUPPORTED
    for M in (1, 5, 17):
        for kern in (0, 1, BATCH):
            assert call(FAST, M=M, flags=kern, K=192, g=64, W=3) == UNSUPPORTED  # K % 128: neither kernel


def test_gemv_fast_prefill_refusals():
    assert call(FAST_PREFILL, N=68) == UNSUPPORTED  # the GEMM layout packs eight columns a word
    assert call(FAST_PREFILL, g=32) == UNSUPPORTED
    assert call(FAST_PREFILL, N=68, tmp=None) == NULL
    assert call(FAST_PREFILL, g=32, y=P + 8) == BAD_ALIGNMENT
    assert call(FAST_PREFILL, N=68, W=1) == BAD_SHAPE


# ---- two faults at once: which check comes first
@pytest.mark.parametrize("name", MATMUL)
def test_order_shape_null_alignment(name):
    assert call(name, x=None, K=0) == BAD_SHAPE
    assert call(name, x=P + 8, g=96) == BAD_SHAPE
    assert call(name, x=P + 8, qw=None) == NULL
    assert call(name, s=None, x=P + 8) == NULL
    assert call(name, y=None, qw=P + 8) == NULL
    assert call(name, x=None, N=0) == OK


def test_order_dequantise():
    assert call(DEQ, y=P + 8, qw=None) == NULL
    assert call(DEQ, y=P + 8, K=12, g=12) == BAD_SHAPE
    assert call(DEQ, y=P + 8, N=0) == OK
    assert call(DEQ_FAST, y=None, N=66) == BAD_SHAPE
