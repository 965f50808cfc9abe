"""Return codes of the attention entry points' host checks (csrc/capi.hip and the launchers behind it), without a GPU: the four
RoPE + append entries, the ten decode-attention entries and the verify step's two.  The pointers are a small aligned HOST buffer,
so every call here has to return BEFORE any launch: each case carries at least one fault, or an empty batch.  No case is a fully
valid call, and AWQ_ERR_LAUNCH (-5) is never an expected code.

The expected codes are literals.  They were fixed by running this file against the library as it stood before the entry points
were folded onto AwqAttnArgs / AwqAppendArgs and one validator per family; the two-fault cases pin the ORDER of the checks, which
differs between entry points (an fp8 entry refuses a head size before it looks at the alignment of q, an fp16 entry after)."""
import ctypes
import math

import pytest

OK, BAD_SHAPE, BAD_ALIGNMENT, UNSUPPORTED, LAUNCH, NULL = 0, -1, -2, -3, -5, -6

_buf = ctypes.create_string_buffer(256)
P = (ctypes.addressof(_buf) + 63) & ~63  # 16-byte aligned, never dereferenced

# the arguments of each entry point in ABI order (include/awq_hip.h), by role: `word` is the device position / length word
# (shared or per-row), `pos` the host seq_len / start_pos
ENTRIES = {
    "awq_rope_kv_append": "qkv q_out k v cos sin word pos B S Hq Hkv D rot Tmax stream",
    "awq_rope_kv_append_rows": "qkv q_out k v cos sin word B S Hq Hkv D rot Tmax stream",
    "awq_rope_kv_append_fp8": "qkv q_out k v ks vs cos sin word pos B S Hq Hkv D rot Tmax stream",
    "awq_rope_kv_append_rows_fp8": "qkv q_out k v ks vs cos sin word B S Hq Hkv D rot Tmax stream",
    "awq_decode_attention": "q k v out word pos max_len B Hq Hkv D Tmax scale ws bytes stream",
    "awq_decode_attention_ex": "q k v out word pos max_len B Hq Hkv D Tmax scale softcap alibi ws bytes stream",
    "awq_decode_attention_rope": "qkv k v cos sin out word pos max_len B Hq Hkv D Tmax scale ws bytes stream",
    "awq_decode_attention_rows": "q k v out word max_len B Hq Hkv D Tmax scale softcap alibi ws bytes stream",
    "awq_decode_attention_rope_rows": "qkv k v cos sin out word max_len B Hq Hkv D Tmax scale ws bytes stream",
    "awq_decode_attention_fp8": "q k v ks vs out word pos max_len B Hq Hkv D Tmax scale ws bytes stream",
    "awq_decode_attention_ex_fp8": "q k v ks vs out word pos max_len B Hq Hkv D Tmax scale softcap alibi ws bytes stream",
    "awq_decode_attention_rope_fp8": "qkv k v ks vs cos sin out word pos max_len B Hq Hkv D Tmax scale ws bytes stream",
    "awq_decode_attention_rows_fp8": "q k v ks vs out word max_len B Hq Hkv D Tmax scale softcap alibi ws bytes stream",
    "awq_decode_attention_rope_rows_fp8": "qkv k v ks vs cos sin out word max_len B Hq Hkv D Tmax scale ws bytes stream",
    "awq_verify_attention_rows": "q k v out word max_len B T Hq Hkv D Tmax scale ws bytes stream",
}
# a call that would be valid (and so is never made as it stands): 2 sequences, 8 query heads on 2 KV heads, a 64-row cache
VALID = dict(qkv=P, q=P, q_out=P, out=P, k=P, v=P, ks=P, vs=P, cos=P, sin=P, word=P, pos=5, max_len=16, B=2, S=1, T=4, Hq=8, Hkv=2,
             D=128, rot=128, Tmax=64, scale=0.125, softcap=0.0, alibi=None, ws=P, bytes=0, stream=None)

APPEND = [n for n in ENTRIES if "append" in n]
DECODE = [n for n in ENTRIES if "decode" in n]
VERIFY = "awq_verify_attention_rows"
FP8 = [n for n in ENTRIES if n.endswith("fp8")]
ROWS = [n for n in ENTRIES if "_rows" in n]
SOFTCAP = [n for n in ENTRIES if "softcap" in ENTRIES[n]]
ROPE_SHARED = ["awq_decode_attention_rope", "awq_decode_attention_rope_fp8"]
PLAIN_SHARED = ["awq_decode_attention", "awq_decode_attention_ex", "awq_decode_attention_fp8", "awq_decode_attention_ex_fp8"]


def call(name, **faults):
    from autoawq_amd import _lib

    roles = ENTRIES[name].split()
    assert faults and set(faults) <= set(roles), (name, faults)
    rc = getattr(_lib.lib(), name)(*[faults.get(r, VALID[r]) for r in roles])
    assert rc != LAUNCH, (name, faults)  # the call got as far as a launch: the case is wrong, not the library
    return rc


def _roles(name, among):
    return [r for r in ENTRIES[name].split() if r in among]


def _cases(names, among):
    return [(n, r) for n in names for r in _roles(n, among)]


def test_the_table_names_every_entry_point():
    from autoawq_amd import _lib

    for name, roles in ENTRIES.items():
        assert len(roles.split()) == len(_lib.SIGNATURES[name][1]), name
    assert len(APPEND) == 4 and len(DECODE) == 10


@pytest.mark.parametrize("name", list(ENTRIES))
def test_empty_batch_is_ok(name):
    assert call(name, B=0) == OK
    assert call(name, B=0, **{r: None for r in _roles(name, ("qkv", "q", "k", "out"))}) == OK  # before the pointer checks
    if name in APPEND:
        assert call(name, S=0) == OK
        assert call(name, S=0, qkv=None) == OK


# ---- required pointers
@pytest.mark.parametrize("name,role", _cases(ENTRIES, ("qkv", "q", "q_out", "out", "k", "v", "ks", "vs", "cos", "sin")))
def test_required_pointer_null(name, role):
    assert call(name, **{role: None}) == NULL


@pytest.mark.parametrize("name", ROWS)
def test_missing_per_row_word(name):
    assert call(name, word=None) == NULL


@pytest.mark.parametrize("name", FP8)
def test_one_scale_without_the_other(name):
    assert call(name, ks=None) == NULL
    assert call(name, vs=None) == NULL


# ---- alignment: the fp16 append entries check none; the fp8 ones their caches and scales; attention q / qkv, caches and out
@pytest.mark.parametrize("name,role", _cases(DECODE + [VERIFY], ("qkv", "q", "k", "v", "out")) + _cases(
    [n for n in APPEND if n in FP8], ("k", "v")))
def test_misaligned_pointer(name, role):
    assert call(name, **{role: P + 8}) == BAD_ALIGNMENT


@pytest.mark.parametrize("name,role", _cases(FP8, ("ks", "vs")))
def test_scale_pointer_off_by_two(name, role):
    assert call(name, **{role: P + 2}) == BAD_ALIGNMENT


# ---- shapes
@pytest.mark.parametrize("name", DECODE + [VERIFY])
def test_attention_batch_out_of_range(name):
    assert call(name, B=-1) == BAD_SHAPE
    assert call(name, B=65536) == BAD_SHAPE


@pytest.mark.parametrize("name", APPEND)
def test_append_batch_out_of_range(name):
    assert call(name, B=-1) == BAD_SHAPE
    assert call(name, S=-1) == BAD_SHAPE
    assert call(name, B=(1 << 21) + 1) == BAD_SHAPE  # B S rows of up to 1024 blocks each: past INT32_MAX
    assert call(name, B=1 << 11, S=(1 << 10) + 1) == BAD_SHAPE
    assert call(name, Tmax=0) == BAD_SHAPE
    assert call(name, Tmax=1 << 31) == BAD_SHAPE
    assert call(name, Tmax=0, B=0) == BAD_SHAPE


@pytest.mark.parametrize("name", DECODE + [VERIFY])
def test_attention_head_dim_not_128(name):
    assert call(name, D=64) == UNSUPPORTED
    assert call(name, D=256) == UNSUPPORTED


@pytest.mark.parametrize("name", APPEND)
def test_append_head_dim(name):
    fp8 = name in FP8
    if fp8:  # (fp16: any even D <= 256 is a valid call)
        assert call(name, D=64, rot=64) == UNSUPPORTED
    assert call(name, D=258) == (UNSUPPORTED if fp8 else BAD_SHAPE)
    assert call(name, D=127) == (UNSUPPORTED if fp8 else BAD_SHAPE)
    assert call(name, rot=130) == BAD_SHAPE
    assert call(name, rot=3) == BAD_SHAPE
    assert call(name, rot=-2) == BAD_SHAPE


@pytest.mark.parametrize("name", ENTRIES)
def test_head_counts(name):
    assert call(name, Hq=0) == BAD_SHAPE
    assert call(name, Hkv=0) == BAD_SHAPE
    if name in APPEND:
        return  # (the append kernels take any ratio)
    assert call(name, Hkv=65536) == BAD_SHAPE
    assert call(name, Hq=6, Hkv=2) == UNSUPPORTED  # 3 query heads per KV head: no kernel
    assert call(name, Hq=32, Hkv=2) == UNSUPPORTED
    assert call(name, Hq=5, Hkv=2) == BAD_SHAPE  # not a whole ratio


@pytest.mark.parametrize("name", SOFTCAP)
def test_softcap_negative_or_nan(name):
    assert call(name, softcap=-1.0) == BAD_SHAPE
    assert call(name, softcap=math.nan) == BAD_SHAPE
    assert call(name, softcap=-math.inf) == BAD_SHAPE


# ---- lengths and positions
@pytest.mark.parametrize("name", DECODE + [VERIFY])
def test_length_beyond_the_cache(name):
    assert call(name, max_len=65) == BAD_SHAPE  # (a device word is given: the launch is sized for max_len)
    assert call(name, max_len=0) == BAD_SHAPE
    assert call(name, Tmax=1 << 31) == BAD_SHAPE
    assert call(name, Tmax=0) == BAD_SHAPE
    if name in PLAIN_SHARED:
        assert call(name, word=None, pos=65) == BAD_SHAPE
        assert call(name, word=None, pos=0) == BAD_SHAPE
    if name == VERIFY:
        assert call(name, max_len=3) == BAD_SHAPE  # below T
        assert call(name, max_len=-1) == BAD_SHAPE
        assert call(name, max_len=1 << 31) == BAD_SHAPE


@pytest.mark.parametrize("name", ROPE_SHARED)
def test_host_start_position_out_of_range(name):
    assert call(name, word=None, pos=-1) == BAD_SHAPE
    assert call(name, word=None, pos=64) == BAD_SHAPE


@pytest.mark.parametrize("name", ["awq_rope_kv_append", "awq_rope_kv_append_fp8"])
def test_append_host_start_position_out_of_range(name):
    assert call(name, word=None, pos=-1) == BAD_SHAPE
    assert call(name, word=None, pos=64) == BAD_SHAPE  # row 64 of a 64-row cache
    assert call(name, word=None, pos=60, S=5) == BAD_SHAPE


def test_verify_token_count_and_grid():
    assert call(VERIFY, T=9) == UNSUPPORTED
    assert call(VERIFY, T=1) == UNSUPPORTED
    assert call(VERIFY, Hq=65536, Hkv=65536) == BAD_SHAPE
    assert call(VERIFY, B=65535, T=8, Hkv=1) == BAD_SHAPE  # 8 token groups per sequence: past the grid's 65535


# ---- two faults at once: which check comes first
def test_order_decode_fp16():
    n = "awq_decode_attention"
    assert call(n, q=None, B=65536) == BAD_SHAPE
    assert call(n, q=None, B=0) == OK
    assert call(n, q=None, k=P + 8) == NULL
    assert call(n, v=None, q=P + 8) == NULL
    assert call(n, q=P + 8, D=64) == BAD_ALIGNMENT  # alignment in the entry point, the head size in the launcher
    assert call(n, D=64, Hq=5) == UNSUPPORTED
    assert call(n, Hq=5, max_len=65) == BAD_SHAPE
    assert call(n, Hq=6, max_len=65) == UNSUPPORTED
    assert call(n, D=64, Tmax=0) == UNSUPPORTED
    assert call(n, out=P + 8, Tmax=1 << 31) == BAD_SHAPE
    for n in ("awq_decode_attention_ex", "awq_decode_attention_rows"):
        assert call(n, softcap=math.nan, B=0) == BAD_SHAPE
        assert call(n, softcap=-1.0, q=None) == BAD_SHAPE
        assert call(n, softcap=-1.0, B=-1) == BAD_SHAPE
    assert call("awq_decode_attention_rows", word=None, q=P + 8) == NULL
    assert call("awq_decode_attention_rows", word=None, D=64) == NULL
    assert call("awq_decode_attention_rope_rows", word=None, k=P + 8) == NULL


def test_order_decode_rope():
    n = "awq_decode_attention_rope"
    assert call(n, word=None, pos=-1, qkv=P + 8) == BAD_ALIGNMENT
    assert call(n, word=None, pos=64, cos=None) == NULL
    assert call(n, word=None, pos=64, D=64) == BAD_SHAPE  # the host position in the entry point, the head size in the launcher
    assert call(n, word=None, pos=64, B=0) == OK
    assert call(n, pos=64, max_len=65) == BAD_SHAPE
    n = "awq_decode_attention_rope_fp8"
    assert call(n, word=None, pos=64, D=64) == UNSUPPORTED  # fp8: the head size with the cache checks, before the position
    assert call(n, word=None, pos=64, qkv=P + 8) == BAD_ALIGNMENT
    assert call(n, word=None, pos=64, ks=None) == NULL


def test_order_decode_fp8():
    for n in ("awq_decode_attention_fp8", "awq_decode_attention_ex_fp8", "awq_decode_attention_rows_fp8"):
        assert call(n, q=P + 8, D=64) == UNSUPPORTED  # fp8: the head size before q's alignment
        assert call(n, ks=None, D=64) == NULL
        assert call(n, k=P + 8, D=64) == UNSUPPORTED
        assert call(n, q=None, vs=P + 2) == NULL
        assert call(n, out=None, D=64) == NULL
        assert call(n, q=P + 8, k=None) == NULL
        assert call(n, ks=None, B=0) == OK
        assert call(n, D=64, B=65536) == BAD_SHAPE
    assert call("awq_decode_attention_rows_fp8", word=None, D=64) == NULL
    assert call("awq_decode_attention_rows_fp8", softcap=-1.0, ks=None) == BAD_SHAPE
    assert call("awq_decode_attention_rope_rows_fp8", word=None, ks=P + 2) == NULL
    assert call("awq_decode_attention_rope_rows_fp8", sin=None, D=64) == NULL


def test_order_verify():
    assert call(VERIFY, T=9, B=0) == UNSUPPORTED
    assert call(VERIFY, T=9, B=65536) == BAD_SHAPE
    assert call(VERIFY, T=9, q=None) == UNSUPPORTED
    assert call(VERIFY, word=None, q=P + 8) == NULL
    assert call(VERIFY, D=64, Hq=5) == BAD_SHAPE  # (the verify launcher checks the ratio before the head size)
    assert call(VERIFY, D=64, max_len=65) == UNSUPPORTED
    assert call(VERIFY, q=P + 8, D=64) == BAD_ALIGNMENT
    assert call(VERIFY, Hq=6, max_len=65) == UNSUPPORTED


def test_order_append():
    n = "awq_rope_kv_append"
    assert call(n, qkv=None, B=-1) == BAD_SHAPE
    assert call(n, qkv=None, S=0) == OK
    assert call(n, cos=None, rot=0, Hq=0) == BAD_SHAPE  # without rotation the tables are not required
    assert call(n, sin=None, Hq=0) == NULL
    assert call(n, word=None, pos=64, v=None) == NULL
    assert call(n, word=None, pos=64, D=258) == BAD_SHAPE
    assert call("awq_rope_kv_append_rows", word=None, Hq=0) == NULL
    assert call("awq_rope_kv_append_rows", word=None, B=0) == OK
    for n in ("awq_rope_kv_append_fp8", "awq_rope_kv_append_rows_fp8"):
        assert call(n, qkv=None, D=64) == NULL
        assert call(n, k=P + 8, D=64) == UNSUPPORTED
        assert call(n, ks=None, D=64) == NULL
        assert call(n, vs=P + 2, Hq=0) == BAD_ALIGNMENT
        assert call(n, D=64, Hq=0) == UNSUPPORTED
        assert call(n, cos=None, rot=0, vs=None) == NULL
    assert call("awq_rope_kv_append_fp8", word=None, pos=64, D=64) == UNSUPPORTED
    assert call("awq_rope_kv_append_rows_fp8", word=None, ks=None) == NULL


# ---- the verify launch's split count: (max_len, B, T, n_heads, n_kv_heads) -> splits
@pytest.mark.parametrize("args,want", [
    ((200, 1, 4, 8, 2), 1),        # up to 256 rows: one split
    ((256, 1, 4, 8, 1), 1),
    ((257, 1, 4, 8, 1), 3),        # then about 128 rows each
    ((1000, 2, 4, 8, 2), 8),
    ((4096, 1, 4, 32, 32), 32),
    ((8192, 1, 2, 8, 8), 64),
    ((100000, 1, 2, 8, 8), 64),    # capped by the combine kernel's 64
    ((4096, 4, 8, 32, 4), 8),      # capped by blocks: 4 sequences x 4 KV heads x 8 token groups
    ((4096, 4, 8, 32, 32), 8),
    ((4096, 64, 8, 32, 32), 1),
    ((0, 1, 4, 8, 2), BAD_SHAPE),
    ((1 << 31, 1, 4, 8, 2), BAD_SHAPE),
    ((4096, 0, 4, 8, 2), BAD_SHAPE),
    ((4096, 65536, 4, 8, 2), BAD_SHAPE),
    ((4096, 1, 9, 8, 2), BAD_SHAPE),
    ((4096, 1, 1, 8, 2), BAD_SHAPE),
    ((4096, 1, 4, 6, 4), BAD_SHAPE),
    ((4096, 1, 4, 8, 0), BAD_SHAPE),
])
def test_verify_attention_splits(args, want):
    from autoawq_amd import _lib

    assert _lib.lib().awq_verify_attention_splits(*args) == want
