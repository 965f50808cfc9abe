"""The opt-in single resident copy of the Mixtral experts on the GPU: awq_repack_gemv_stack_to_gemm (csrc/repack.hip) as the exact
inverse of utils/convert.py::gemm_stack_to_gemv with the experts to convert picked on the device, FusedSparseMoeBlock on one copy
against the same block on two copies (bit for bit: the same kernels on the same integers) and against the oracle, what the block
keeps resident, and fuse_mixtral(expert_copies=1) through GraphedDecoder.generate.
Shape: E = 8, H = 512, I = 768, g = 128 as tests/test_gpu_moe_rows.py -- w1|w3 K = 512, N = 1536; w2 K = 768, N = 512, whose
K / g = 6 is no multiple of 8: the padded zero words and scales of the GEMV layout are in play."""
import numpy as np
import pytest
import torch

from test_gpu_moe_rows import Stack, gemm_stacks

pytestmark = pytest.mark.gpu

E, H, I, G, TOPK = 8, 512, 768, 128, 2
TOUCHED = (0, 3, 7)
SENTINEL = 0x5A5A5A5A  # as int32 words; the fp16 scales hold its halves


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()  # fails loudly if the extension is missing
    return _ops


@pytest.fixture(scope="module")
def stacks():
    """the GEMM-layout stacks (w1|w3, w2) on the device; never written"""
    w1, w2 = gemm_stacks(E, H, I, G, seed=31)
    out = []
    for src in (w1, w2):
        s = Stack()
        s.qweight, s.qzeros, s.scales = src.qweight.cuda(), src.qzeros.cuda(), src.scales.cuda()
        out.append(s)
    return out[0], out[1], w1, w2


@pytest.fixture()
def same_hand_over(monkeypatch):
    """Bit-for-bit parity is a statement about the same kernels on the same integers: both modes hand over from the row-streaming
    kernel at the same pair count here (single-copy mode may keep it for more pairs, moe.ROWS_MAX_PAIRS_SINGLE)."""
    from autoawq_amd.modules.fused import moe

    monkeypatch.setattr(moe, "ROWS_MAX_PAIRS_SINGLE", moe.ROWS_MAX_PAIRS)
    return moe


def _sentinel_like(t):
    return torch.full(t.shape, SENTINEL, dtype=torch.int32, device="cuda") if t.dtype == torch.int32 else \
        torch.full(t.shape[:-1] + (t.shape[-1] // 2,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float16)


def _selectors(n_experts, touched):
    counts = torch.zeros(n_experts, dtype=torch.int32)
    for i, e in enumerate(touched):
        counts[e] = 2 * i + 1
    seg = torch.zeros(n_experts + 1, dtype=torch.int32)
    seg[1:] = torch.cumsum(counts, 0)
    ids = torch.tensor([touched[i % len(touched)] for i in (2, 0, 1, 1, 0)] + [n_experts + 5, -1], dtype=torch.int32)  # + ids of no expert
    return seg.cuda(), ids.view(-1, 1).cuda()


def _round_trip(ops, qweight, qzeros, scales, interleave, touched, n_experts):
    """GEMM layout -> gemm_stack_to_gemv -> the kernel, for the three selectors; qweight / qzeros / scales are on the device"""
    from autoawq_amd.utils.convert import gemm_stack_to_gemv

    t = gemm_stack_to_gemv(qweight, qzeros, scales, interleave_halves=interleave)
    g = t.group_size
    seg, ids = _selectors(n_experts, touched)
    for name, sel, conv in (("all", {}, range(n_experts)), ("seg_offsets", dict(seg_offsets=seg), touched), ("topk_ids", dict(topk_ids=ids), touched)):
        out = (_sentinel_like(qweight), _sentinel_like(scales), _sentinel_like(qzeros))
        qw, sc, qz = ops.repack_gemv_stack_to_gemm(t.qweight, t.scales, t.qzeros, g, out=out, deinterleave_halves=interleave, **sel)
        assert qw.data_ptr() == out[0].data_ptr()
        for e in range(n_experts):
            if e in conv:
                assert torch.equal(qw[e], qweight[e]), (name, e, "qweight")
                assert torch.equal(qz[e], qzeros[e]), (name, e, "qzeros")
                assert torch.equal(sc[e].view(torch.int16), scales[e].view(torch.int16)), (name, e, "scales")
            else:  # not a byte written
                assert bool((qw[e] == SENTINEL).all()) and bool((qz[e] == SENTINEL).all()), (name, e)
                assert bool((sc[e].view(torch.int32) == SENTINEL).all()), (name, e)
    # an empty id list touches no expert
    out = (_sentinel_like(qweight), _sentinel_like(scales), _sentinel_like(qzeros))
    ops.repack_gemv_stack_to_gemm(t.qweight, t.scales, t.qzeros, g, out=out, deinterleave_halves=interleave, topk_ids=ids[:0])
    assert all(bool((o.view(torch.int32) == SENTINEL).all()) for o in out)


@pytest.mark.parametrize("interleave", [True, False])
@pytest.mark.parametrize("which", ["w1w3", "w2"])
def test_stack_repack_inverts_gemm_stack_to_gemv(ops, stacks, which, interleave):
    s = stacks[0] if which == "w1w3" else stacks[1]
    _round_trip(ops, s.qweight, s.qzeros, s.scales, interleave, TOUCHED, E)


@pytest.mark.parametrize("interleave", [True, False])
def test_stack_repack_ragged_tiles(ops, interleave):
    """K / 8 = 48 words and N = 520 columns: neither a multiple of the 32-word x 256-column tile, N / 2 = 260 no multiple of the
    eight columns of an output word (the row map is per column), K / g = 3"""
    n, K, N, g = 3, 384, 520, 128
    gen = torch.Generator().manual_seed(77)
    lim = 2 ** 31 - 1
    qw = torch.randint(-lim - 1, lim, (n, K, N // 8), dtype=torch.int32, generator=gen).cuda()
    qz = torch.randint(-lim - 1, lim, (n, K // g, N // 8), dtype=torch.int32, generator=gen).cuda()
    sc = (torch.rand((n, K // g, N), generator=gen) * 0.02 + 0.005).half().cuda()
    _round_trip(ops, qw, qz, sc, interleave, (1,), n)


def test_stack_repack_refuses_bad_calls(ops, stacks):
    from autoawq_amd.utils.convert import gemm_stack_to_gemv

    s = stacks[1]
    t = gemm_stack_to_gemv(s.qweight, s.qzeros, s.scales)
    seg, ids = _selectors(E, TOUCHED)
    with pytest.raises(Exception, match="code -1"):  # both selectors
        ops.repack_gemv_stack_to_gemm(t.qweight, t.scales, t.qzeros, G, seg_offsets=seg, topk_ids=ids)
    with pytest.raises(Exception):  # out of another shape
        ops.repack_gemv_stack_to_gemm(t.qweight, t.scales, t.qzeros, G, out=(s.qweight[:4], s.scales[:4], s.qzeros[:4]))
    with pytest.raises(Exception):
        ops.repack_gemv_stack_to_gemm(t.qweight.cpu(), t.scales.cpu(), t.qzeros.cpu(), G)


def _blocks(stacks):
    """(two-copy block, one-copy block, the twins) over the same weights and the same router"""
    from autoawq_amd.modules.fused import moe

    a, b = Stack(), Stack()
    for dst, src in ((a, stacks[0]), (b, stacks[1])):
        dst.qweight, dst.qzeros, dst.scales = src.qweight, src.qzeros, src.scales
    t1, t2 = moe.build_decode_twins(a, b)
    assert t1 is not None and t2 is not None
    torch.manual_seed(3)
    gate = torch.nn.Linear(H, E, bias=False).half().cuda()
    two = moe.FusedSparseMoeBlock(TOPK, gate, a, b)
    one = moe.FusedSparseMoeBlock(TOPK, gate, *moe.build_single_copy(a, b))
    return two, one, (t1, t2)


PATHS = {1: "gemv_rows_grouped", 4: "gemv_rows_grouped", 6: "gemv_rows_grouped", 7: "gemv_mfma_grouped", 40: "gemv_mfma_grouped",
         256: "gemm_regb_grouped"}


@pytest.mark.parametrize("T", sorted(PATHS))
def test_block_on_one_copy_equals_block_on_two_copies(ops, stacks, same_hand_over, T):
    two, one, _ = _blocks(stacks)
    x = torch.randn((1, T, H), generator=torch.Generator().manual_seed(T)).half().cuda()
    with torch.inference_mode():
        want = two(x)
        k2 = ops.last_kernel()
        got = one(x)
        k1 = ops.last_kernel()
    assert k1 == k2 == PATHS[T], (k1, k2)
    assert torch.equal(got, want)
    assert torch.equal(one(x), got), "not reproducible (the workspace is reused)"


def test_one_copy_prefill_vs_oracle(ops, oracle, stacks):
    from autoawq_amd.modules.fused import moe

    _, one, _ = _blocks(stacks)
    w1, w2 = stacks[2], stacks[3]
    T = 256
    gen = torch.Generator().manual_seed(T)
    x = torch.randn((T, H), generator=gen).half()
    logits = torch.randn((T, E), generator=gen)
    got = moe.apply_moe_weights(one.ws, one.w2s, x.cuda(), logits.cuda(), TOPK, True)
    assert ops.last_kernel() == "gemm_regb_grouped"
    want, _, _ = oracle.moe_forward(x.numpy(), logits.numpy(), dict(qweight=w1.qweight.numpy(), qzeros=w1.qzeros.numpy(), scales=w1.scales.numpy()),
                                    dict(qweight=w2.qweight.numpy(), qzeros=w2.qzeros.numpy(), scales=w2.scales.numpy()), TOPK, G)
    w64 = want.astype(np.float64)
    rms = np.sqrt((w64 ** 2).mean())
    err = np.abs(got.cpu().numpy().astype(np.float64) - w64)
    print("one-copy prefill vs oracle: max err / rms", err.max() / rms)
    assert (err <= 4e-3 * np.abs(w64) + 4e-3 * rms).all(), err.max() / rms  # the bound of test_gpu_moe_rows.py for this shape


def test_one_copy_keeps_the_twins_bytes_alone_and_follows_to(ops, stacks, same_hand_over):
    from autoawq_amd.utils.convert import ExpertStackResident

    moe = same_hand_over
    two, one, twins = _blocks(stacks)
    nbytes = lambda t: sum(b.numel() * b.element_size() for b in (t.qweight, t.qzeros, t.scales))
    assert one.expert_bytes() == nbytes(twins[0]) + nbytes(twins[1])
    assert two.expert_bytes() == one.expert_bytes() + nbytes(stacks[0]) + nbytes(stacks[1])
    # nothing in the GEMM layout is reachable from the block: its only expert tensors are the six registered GEMV-layout buffers
    assert isinstance(one.ws, ExpertStackResident) and isinstance(one.w2s, ExpertStackResident)
    assert not hasattr(one.ws, "decode_twin") and not hasattr(one.w2s, "decode_twin")
    big = {n: tuple(b.shape) for n, b in one.named_buffers() if b.dim() == 3}
    assert sorted(big) == ["w2s.qweight", "w2s.qzeros", "w2s.scales", "ws.qweight", "ws.qzeros", "ws.scales"]
    assert big["ws.qweight"] == (E, 2 * I, H // 8) and big["w2s.qweight"] == (E, H, I // 8)
    assert sum(b.numel() * b.element_size() for n, b in one.named_buffers() if b.dim() == 3) == one.expert_bytes()
    assert not [v for m in one.modules() for v in vars(m).values() if torch.is_tensor(v) and v.dim() == 3]
    # .to() moves the single copy; a block left on another device says so instead of launching
    xs = {T: torch.randn((1, T, H), generator=torch.Generator().manual_seed(100 + T)).half().cuda() for T in (2, 20, 200)}
    with torch.inference_mode():
        before = {T: one(x) for T, x in xs.items()}
    one.to("cpu")
    assert not one.ws.qweight.is_cuda and not one.w2s.scales.is_cuda
    with pytest.raises(RuntimeError, match="single-copy expert stacks are on cpu"):
        moe.apply_moe_weights(one.ws, one.w2s, xs[2][0], torch.zeros((2, E), device="cuda"), TOPK, True)
    one.to("cuda")
    with torch.inference_mode():
        for T, x in xs.items():
            assert torch.equal(one(x), before[T]), T


@pytest.mark.parametrize("batch", [1, 8])
def test_fuse_mixtral_single_copy_generates_the_same_ids(ops, same_hand_over, batch):
    """GraphedDecoder.generate, greedy, 8 tokens: batch 1 decodes on the row-streaming kernel, batch 8 (16 pairs) repacks inside the
    captured step (the mid path); the prompt (5 tokens: 10 / 80 pairs) is prefilled eagerly through the mid path."""
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral
    from autoawq_amd.modules.fused.decode import GraphedDecoder
    from autoawq_amd.utils.convert import ExpertStackResident

    ids = torch.randint(0, test_mixtral.V, (batch, 5), generator=torch.Generator().manual_seed(batch)).cuda()
    out = []
    for copies in (2, 1):
        lm = fuse_mixtral(test_mixtral.build().cuda(), max_seq_len=32, expert_copies=copies)
        if copies == 1:
            assert lm.decode_layout == "gemv (attention projections, experts: single copy)"
            assert all(isinstance(b.moe.ws, ExpertStackResident) for b in lm.model.blocks)
        else:
            assert lm.decode_layout == "gemv (attention projections, expert twins for decode) + gemm (experts)"
        dec = GraphedDecoder(lm, batch=batch, buckets=(16, 32))
        out.append(dec.generate(ids, 8))
    assert out[0].shape == (batch, 13) and torch.equal(out[0], out[1])
