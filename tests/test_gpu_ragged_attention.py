"""Per-row decode kernels (awq_rope_kv_append_rows, awq_decode_attention_rows, awq_decode_attention_rope_rows): every sequence
of the batch reads its own position / length.  Each row must be BITWISE equal to the shared-word kernel run on that row alone
with the same max_len (output and cache rows written), and close to the fp64 oracle.  The positions cover row 0, 1, both
sides of the 256-row single-split boundary, a row deep in a multi-split bucket and the last cache row; short rows in a long
bucket leave splits of the launch empty."""
import numpy as np
import pytest
import torch

import attn_bound

pytestmark = pytest.mark.gpu

TMAX = 1024
POSITIONS = [0, 1, 255, 256, 700, TMAX - 1]   # 0-based position of the new token; length = position + 1
GROUPS = [1, 2, 4, 8]
HKV = 2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()
    return _ops


def _close(got, want):
    assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 2 ** -11


def _caches(gen, B, Tmax=TMAX, Hkv=HKV):
    kc = torch.randn((B, Tmax, Hkv, 128), generator=gen).half()
    vc = torch.randn((B, Tmax, Hkv, 128), generator=gen).half()
    return kc.cuda(), vc.cuda()


def _rows(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("softcap,alibi", [(0.0, False), (30.0, False), (0.0, True), (8.0, True)])
@pytest.mark.parametrize("max_len", [TMAX, 300])
def test_decode_attention_rows_equals_each_row_alone(ops, G, softcap, alibi, max_len):
    from oracle import decoder_oracle

    lens = [p + 1 for p in POSITIONS if p + 1 <= max_len]
    B, Hq = len(lens), HKV * G
    gen = torch.Generator().manual_seed(G * 100 + int(softcap) + 7 * alibi + max_len)
    q = (torch.randn((B, Hq, 128), generator=gen) * 2).half().cuda()
    kc, vc = _caches(gen, B)
    for b, n in enumerate(lens):   # rows past a sequence's length must not be read
        kc[b, n:] = 100.0
        vc[b, n:] = 100.0
    slopes = decoder_oracle.alibi_slopes_reference(Hq) if alibi else None
    sl = torch.from_numpy(slopes).float().cuda() if alibi else None
    got = ops.decode_attention(q, kc, vc, 1, max_len=max_len, softcap=softcap, alibi_slopes=sl, len_rows=_rows(lens))
    for b, n in enumerate(lens):
        alone = ops.decode_attention(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], 1, len_dev=_rows([n]), max_len=max_len,
                                     softcap=softcap, alibi_slopes=sl)
        assert torch.equal(got[b:b + 1], alone), (b, n)
        want = decoder_oracle.attention_reference(q[b:b + 1].cpu().numpy(), kc[b:b + 1].cpu().numpy(),
                                                  vc[b:b + 1].cpu().numpy(), n, softcap=softcap, alibi_slopes=slopes)
        _close(got[b:b + 1].cpu().numpy().astype(np.float64), want)
        w, bound = attn_bound.decode_bound(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], [n], attn_bound.decode_splits(max_len, B, Hq, HKV),
                                           softcap=softcap, alibi=sl)
        attn_bound.assert_attention_close(got[b:b + 1], w, bound, f"row {b} length {n}")


@pytest.mark.parametrize("G", GROUPS)
def test_decode_attention_rope_rows_equals_each_row_alone(ops, G):
    from autoawq_amd.modules.fused.attn import RoPE
    from oracle import decoder_oracle

    B, Hq = len(POSITIONS), HKV * G
    gen = torch.Generator().manual_seed(G)
    qkv = torch.randn((B, 1, (Hq + 2 * HKV) * 128), generator=gen).half().cuda()
    kc, vc = _caches(gen, B)
    rope = RoPE(128, TMAX, "cuda", 10000.0)
    k0, v0 = kc.clone(), vc.clone()
    got = ops.decode_attention_rope(qkv, kc, vc, rope.cos, rope.sin, 0, Hq, HKV, max_len=TMAX, pos_rows=_rows(POSITIONS))
    for b, p in enumerate(POSITIONS):
        ka, va = k0[b:b + 1].clone(), v0[b:b + 1].clone()
        alone = ops.decode_attention_rope(qkv[b:b + 1], ka, va, rope.cos, rope.sin, 0, Hq, HKV, pos_dev=_rows([p]), max_len=TMAX)
        assert torch.equal(got[b:b + 1], alone), (b, p)
        assert torch.equal(kc[b:b + 1], ka) and torch.equal(vc[b:b + 1], va), (b, p)   # the append, and nothing else
        # the oracle on the appended cache: the new query (rotated like the append kernel rotates) over rows [0, p]
        q = ops.rope_kv_append(qkv[b:b + 1], ka.clone(), va.clone(), rope.cos, rope.sin, p, Hq, HKV, 128, 128)
        want = decoder_oracle.attention_reference(q[:, 0].cpu().numpy(), ka.cpu().numpy(), va.cpu().numpy(), p + 1)
        _close(got[b:b + 1].cpu().numpy().astype(np.float64), want)
        w, bound = attn_bound.decode_bound(q[:, 0], ka, va, [p + 1], attn_bound.decode_splits(TMAX, B, Hq, HKV))
        attn_bound.assert_attention_close(got[b:b + 1], w, bound, f"row {b} position {p}")


@pytest.mark.parametrize("rot", [128, 64])
@pytest.mark.parametrize("S", [1, 3])
def test_rope_kv_append_rows_equals_each_row_alone(ops, rot, S):
    """Partial rotary included; S > 1 clamps the last rows of the row at Tmax - 1 the way the shared kernel does."""
    from autoawq_amd.modules.fused.attn import RoPE

    Hq, B = 4, len(POSITIONS)
    gen = torch.Generator().manual_seed(rot + S)
    qkv = torch.randn((B, S, (Hq + 2 * HKV) * 128), generator=gen).half().cuda()
    kc, vc = _caches(gen, B)
    rope = RoPE(rot, TMAX, "cuda", 10000.0)
    k0, v0 = kc.clone(), vc.clone()
    q = ops.rope_kv_append(qkv, kc, vc, rope.cos, rope.sin, 0, Hq, HKV, 128, rot, pos_rows=_rows(POSITIONS))
    for b, p in enumerate(POSITIONS):
        ka, va = k0[b:b + 1].clone(), v0[b:b + 1].clone()
        qa = ops.rope_kv_append(qkv[b:b + 1], ka, va, rope.cos, rope.sin, 0, Hq, HKV, 128, rot, pos_dev=_rows([p]))
        # (p + S > Tmax: several tokens of the row are clamped onto cache row Tmax - 1 -- which of them lands there is not
        #  specified, in either form; every other row is)
        rows = slice(0, TMAX - 1) if p + S > TMAX else slice(0, TMAX)
        assert torch.equal(q[b:b + 1], qa), (b, p)
        assert torch.equal(kc[b:b + 1, rows], ka[:, rows]) and torch.equal(vc[b:b + 1, rows], va[:, rows]), (b, p)


def test_short_rows_in_a_long_bucket_leave_empty_splits(ops):
    """max_len 4096 gives the launch 32 splits; rows of length 1, 2 and 17 fill only the first of them.  The empty splits
    must contribute nothing: the result equals the single-split launch of the same rows (max_len = length)."""
    lens = [1, 2, 17]
    B, Hq = 3, 8
    gen = torch.Generator().manual_seed(5)
    q = torch.randn((B, Hq, 128), generator=gen).half().cuda()
    kc, vc = _caches(gen, B, Tmax=4096)
    for b, n in enumerate(lens):
        kc[b, n:] = float("nan")   # never read, never weighted
        vc[b, n:] = float("nan")
    got = ops.decode_attention(q, kc, vc, 1, max_len=4096, len_rows=_rows(lens))
    assert not bool(got.isnan().any())
    for b, n in enumerate(lens):
        single = ops.decode_attention(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], n)
        assert (got[b:b + 1].float() - single.float()).abs().max().item() <= 2e-3 * single.float().abs().max().item() + 2 ** -11
        w, bound = attn_bound.decode_bound(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], [n], attn_bound.decode_splits(4096, B, Hq, HKV))
        attn_bound.assert_attention_close(got[b:b + 1], w, bound, f"row {b} length {n} of a 4096 bucket")


def test_argument_checks(ops):
    from autoawq_amd._lib import AwqHipError

    q = torch.zeros((2, 4, 128), dtype=torch.float16, device="cuda")
    kc = torch.zeros((2, 64, 2, 128), dtype=torch.float16, device="cuda")
    for bad in (_rows([3]), torch.tensor([3, 4], dtype=torch.int64, device="cuda"), torch.tensor([3, 4], dtype=torch.int32)):
        with pytest.raises(AwqHipError):
            ops.decode_attention(q, kc, kc, 1, len_rows=bad)
    with pytest.raises(AwqHipError):   # not together with the shared word
        ops.decode_attention(q, kc, kc, 1, len_dev=_rows([3]), len_rows=_rows([3, 4]))


def test_rows_step_in_a_hip_graph(ops):
    """One fused per-row step captured with the [B] words advanced on the device; two replays equal the eager per-row calls."""
    from autoawq_amd.modules.fused.attn import RoPE

    G, Hq = 4, 8
    pos0 = [0, 255, 700]
    B = len(pos0)
    gen = torch.Generator().manual_seed(9)
    qkv = torch.randn((B, 1, (Hq + 2 * HKV) * 128), generator=gen).half().cuda()
    kc, vc = _caches(gen, B)
    rope = RoPE(128, TMAX, "cuda", 10000.0)
    k0, v0 = kc.clone(), vc.clone()
    pos = _rows(pos0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.decode_attention_rope(qkv, kc, vc, rope.cos, rope.sin, 0, Hq, HKV, max_len=TMAX, pos_rows=pos)  # warm-up
        torch.cuda.synchronize()
        kc.copy_(k0)
        vc.copy_(v0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = ops.decode_attention_rope(qkv, kc, vc, rope.cos, rope.sin, 0, Hq, HKV, max_len=TMAX, pos_rows=pos)
            pos.add_(1)
    torch.cuda.current_stream().wait_stream(s)
    pos.copy_(_rows(pos0))
    kr, vr = k0.clone(), v0.clone()
    for step in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want = ops.decode_attention_rope(qkv, kr, vr, rope.cos, rope.sin, 0, Hq, HKV, max_len=TMAX,
                                         pos_rows=_rows([p + step for p in pos0]))
        assert torch.equal(out, want) and torch.equal(kc, kr) and torch.equal(vc, vr), step
    assert pos.tolist() == [p + 2 for p in pos0]
