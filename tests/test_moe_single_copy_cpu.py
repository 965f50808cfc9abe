"""The opt-in single resident copy of the Mixtral experts, host side (no GPU): the return codes of awq_repack_gemv_stack_to_gemm's
host checks (csrc/repack.hip; every refusal comes before any launch, so the pointers are a small aligned HOST buffer that is never
dereferenced, in the style of test_gemm_abi_cpu.py) and fuse_mixtral's `expert_copies` keyword on the tiny Mixtral of
test_mixtral.py."""
import ctypes

import pytest
import torch

OK, BAD_SHAPE, BAD_ALIGNMENT, LAUNCH, NULL = 0, -1, -2, -5, -6
DEINTERLEAVE = 1  # AWQ_REPACK_DEINTERLEAVE_HALVES

_buf = ctypes.create_string_buffer(256)
P = (ctypes.addressof(_buf) + 63) & ~63  # 16-byte aligned, never dereferenced

ROLES = "qw s qz qw_out s_out qz_out seg ids pairs E K N g zw flags stream".split()
# a call that would be valid (and so is never made as it stands): four experts of a 256 x 64 matrix in groups of 128, every expert
VALID = dict(qw=P, s=P, qz=P, qw_out=P, s_out=P, qz_out=P, seg=None, ids=None, pairs=0, E=4, K=256, N=64, g=128, zw=1, flags=0,
             stream=None)


def call(**faults):
    from autoawq_amd import _lib

    assert faults and set(faults) <= set(ROLES), faults
    v = {r: faults.get(r, VALID[r]) for r in ROLES}
    rc = _lib.lib().awq_repack_gemv_stack_to_gemm(*[v[r] for r in ROLES])
    assert rc != LAUNCH, faults  # the call got as far as a launch: the case is wrong, not the library
    if rc == OK:  # only a call with nothing to convert may succeed here: anything else ran a kernel on the host buffer
        assert v["E"] == 0 or (v["ids"] is not None and v["pairs"] == 0), faults
    return rc


def test_the_table_matches_the_ctypes_signature():
    from autoawq_amd import _lib

    assert len(ROLES) == len(_lib.SIGNATURES["awq_repack_gemv_stack_to_gemm"][1])


@pytest.mark.parametrize("role", ["qw", "s", "qz", "qw_out", "s_out", "qz_out"])
def test_null_buffer(role):
    assert call(**{role: None}) == NULL
    assert call(**{role: None}, flags=DEINTERLEAVE) == NULL
    assert call(**{role: None}, seg=P) == NULL


def test_shape_rule():
    assert call(N=68) == BAD_SHAPE            # N % 8
    assert call(N=12) == BAD_SHAPE
    assert call(g=96) == BAD_SHAPE            # K % group_size
    assert call(K=200) == BAD_SHAPE
    assert call(g=0) == BAD_SHAPE
    assert call(K=-256) == BAD_SHAPE
    assert call(N=0) == BAD_SHAPE
    assert call(zw=0) == BAD_SHAPE
    assert call(K=4096, zw=3) == BAD_SHAPE    # 8 zw < K / g
    assert call(K=1 << 31) == BAD_SHAPE
    assert call(N=1 << 31) == BAD_SHAPE
    assert call(E=-1) == BAD_SHAPE
    assert call(E=65536) == BAD_SHAPE
    assert call(ids=P, pairs=-1) == BAD_SHAPE
    assert call(flags=2) == BAD_SHAPE         # an unknown flag bit
    # the shape rule comes before the pointers, as in awq_repack_gemv_to_gemm
    assert call(N=68, qw=None) == BAD_SHAPE
    assert call(g=96, s_out=P + 8) == BAD_SHAPE


def test_misaligned_pointers():
    assert call(s_out=P + 8) == BAD_ALIGNMENT  # the scales are written in 16-byte stores
    assert call(s_out=P + 2) == BAD_ALIGNMENT
    assert call(qw=P + 2) == BAD_ALIGNMENT     # packed words
    assert call(qw=P + 1, seg=P) == BAD_ALIGNMENT
    assert call(s_out=P + 8, qz=None) == NULL  # NULL before the alignment


def test_both_selectors_given():
    assert call(seg=P, ids=P, pairs=2) == BAD_SHAPE
    assert call(seg=P, ids=P, pairs=0) == BAD_SHAPE
    assert call(seg=P, ids=P, E=0) == BAD_SHAPE
    assert call(seg=P, ids=P, pairs=2, qw=None) == BAD_SHAPE


def test_nothing_to_convert_is_ok():
    assert call(E=0) == OK
    assert call(E=0, seg=P) == OK
    assert call(E=0, flags=DEINTERLEAVE) == OK
    assert call(ids=P, pairs=0) == OK
    assert call(ids=P, pairs=0, flags=DEINTERLEAVE) == OK
    # ... but only after the checks every call gets
    assert call(E=0, N=68) == BAD_SHAPE
    assert call(E=0, qw=None) == NULL
    assert call(ids=P, pairs=0, s_out=P + 8) == BAD_ALIGNMENT


def test_single_copy_needs_a_decode_layout():
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral

    with pytest.raises(ValueError, match="decode_layout"):
        fuse_mixtral(test_mixtral.build(), max_seq_len=32, decode_layout=None, expert_copies=1)


def test_expert_copies_other_than_1_or_2_is_refused():
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral

    for bad in (3, 0, "1"):
        with pytest.raises(ValueError, match="expert_copies"):
            fuse_mixtral(test_mixtral.build(), max_seq_len=32, expert_copies=bad)


def test_expert_copies_absent_is_two_copies():
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral
    from autoawq_amd.modules.linear import WQLinear_GEMM

    a = fuse_mixtral(test_mixtral.build(), max_seq_len=32)
    b = fuse_mixtral(test_mixtral.build(), max_seq_len=32, expert_copies=2)
    assert a.decode_layout == b.decode_layout == "gemv (attention projections) + gemm (experts)"  # (on the CPU no twins are built)
    for x, y in zip(a.model.blocks, b.model.blocks):
        for name in ("ws", "w2s"):
            sx, sy = getattr(x.moe, name), getattr(y.moe, name)
            assert type(sx) is type(sy) is WQLinear_GEMM and getattr(sx, "layout", None) is None
            for buf in ("qweight", "qzeros", "scales"):
                assert torch.equal(getattr(sx, buf), getattr(sy, buf))
    E, H, I = test_mixtral.E, test_mixtral.H, test_mixtral.I
    assert a.model.blocks[0].moe.ws.qweight.shape == (E, H, 2 * I // 8) and a.model.blocks[0].moe.w2s.qweight.shape == (E, I, H // 8)
    assert sorted(a.state_dict()) == sorted(b.state_dict())


def test_single_copy_structure_and_refused_shapes():
    """expert_copies=1 on the CPU (the conversion is plain torch): the block holds two ExpertStackResident with registered buffers and
    no GEMM-layout stack; a shape the row-streaming kernel does not take is a ValueError that names it, not a fallback."""
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral
    from autoawq_amd.modules.fused import moe
    from autoawq_amd.utils.convert import ExpertStackResident, gemm_stack_to_gemv

    ref = fuse_mixtral(test_mixtral.build(), max_seq_len=32)
    lm = fuse_mixtral(test_mixtral.build(), max_seq_len=32, expert_copies=1)
    assert lm.decode_layout == "gemv (attention projections, experts: single copy)"
    E, H, I = test_mixtral.E, test_mixtral.H, test_mixtral.I
    for blk, rblk in zip(lm.model.blocks, ref.model.blocks):
        ws, w2s = blk.moe.ws, blk.moe.w2s
        assert isinstance(ws, ExpertStackResident) and isinstance(w2s, ExpertStackResident)
        assert ws.layout == w2s.layout == "gemv" and ws.interleaved and not w2s.interleaved and ws.group_size == w2s.group_size == 128
        assert ws.qweight.shape == (E, 2 * I, H // 8) and w2s.qweight.shape == (E, H, I // 8)
        assert sorted(n for n, _ in ws.named_buffers()) == ["qweight", "qzeros", "scales"]
        want = gemm_stack_to_gemv(rblk.moe.ws.qweight, rblk.moe.ws.qzeros, rblk.moe.ws.scales, interleave_halves=True)
        assert torch.equal(ws.qweight, want.qweight) and torch.equal(ws.qzeros, want.qzeros) and torch.equal(ws.scales, want.scales)
        # every expert tensor reachable from the block is a GEMV-layout one ([E, N, ...]: dim 1 = the output rows)
        shapes = [tuple(b.shape) for n, b in blk.moe.named_buffers() if b.dim() == 3]
        assert len(shapes) == 6 and all(s[1] in (2 * I, H) and s[0] == E for s in shapes)
        assert blk.moe.expert_bytes() == ws.expert_bytes() + w2s.expert_bytes()
    # no CPU path behind it either
    from autoawq_amd._lib import AwqHipError

    with pytest.raises(AwqHipError):
        lm.model.blocks[0].moe(torch.zeros((1, 1, H), dtype=torch.float16))

    class Stack:
        pass
    a, b = Stack(), Stack()
    a.qweight, a.qzeros = torch.zeros((2, 128, 16), dtype=torch.int32), torch.zeros((2, 2, 16), dtype=torch.int32)   # K = 128, g = 64
    b.qweight, b.qzeros = torch.zeros((2, 128, 16), dtype=torch.int32), torch.zeros((2, 1, 16), dtype=torch.int32)
    with pytest.raises(ValueError, match="K = 128, group_size = 64"):
        moe.build_single_copy(a, b)
