"""Prefill at per-row positions, kernel level: awq_prefill_attention_rows and awq_rope_kv_append_rows_n[_fp8] through direct ops
calls.  Six rows whose (position, count) cover a single query, counts that cross the 128-row block and the 32-row wave, a start
that is no tile multiple, an end exactly at the cache's last row, and an empty row.  Real slots are held to the derived bound of
tests/attn_bound.py against the fp64 reference, each row with its own start; pad slots and the empty row must keep the sentinel
bit for bit."""
import pytest
import torch

import attn_bound as ab
import attn_needles as nd

pytestmark = pytest.mark.gpu

D = 128
HKV = 2
TMAX = 512
ROWS = [(0, 1), (0, 130), (127, 2), (200, 129), (383, 129), (77, 0)]
S = 130
SENTINEL = 0x7B2A   # an fp16 bit pattern no kernel output takes by accident (58688.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()
    return _ops


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _sentinel(shape, dtype=torch.float16):
    if dtype == torch.float16:
        return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    return torch.full(shape, -12345.5, dtype=dtype, device="cuda")


_CASES = {}


def _case(G):
    """q [6, S, Hq, D], caches [6, TMAX, HKV, D] and targets, built once per G: row b is prefill_needles at its own start; cache rows
    at and above its end are NaN, the query slots behind its count random"""
    if G not in _CASES:
        Hq = HKV * G
        gen = torch.Generator().manual_seed(7 + G)
        q = nd.pm1(gen, (len(ROWS), S, Hq, D)) * 2
        k = torch.empty((len(ROWS), TMAX, HKV, D), dtype=torch.float16)
        v = torch.empty_like(k)
        tgt = []
        for b, (pos, cnt) in enumerate(ROWS):
            qb, kb, vb, tb = nd.prefill_needles(1, max(cnt, 1), Hq, HKV, pos, TMAX, seed=100 * G + b)
            k[b], v[b] = kb[0], vb[0]
            q[b, :cnt] = qb[0, :cnt]
            if pos > 0 and cnt > 0:   # one needle on the row just below the start: the last head of query 0
                q[b, 0, Hq - 1] = (2.0 * kb[0, pos - 1, (Hq - 1) // G].float()).half()
                tb[0, 0, Hq - 1] = pos - 1
            k[b, pos + cnt:] = float("nan")
            v[b, pos + cnt:] = float("nan")
            tgt.append(tb[:, :cnt])
        _CASES[G] = (q.cuda(), k.cuda(), v.cuda(), tgt)
    return _CASES[G]


def _run(ops, q, k, v, pos, cnt, max_end=TMAX, **kw):
    out = _sentinel(q.shape)
    got = ops.prefill_attention_rows(q, k, v, _i32(pos), _i32(cnt), max_end, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return out


@pytest.mark.parametrize("G", [1, 4])
def test_rows_against_the_reference_with_needles(ops, G):
    q, k, v, tgt = _case(G)
    out = _run(ops, q, k, v, [p for p, _ in ROWS], [c for _, c in ROWS])
    bits = out.view(torch.int16)
    # one launch from the wrong start (a row earlier, where there is one): the needle at pos - 1 and the diagonal must show it
    shifted = _run(ops, q, k, v, [max(p - 1, 0) for p, _ in ROWS], [c for _, c in ROWS])
    for b, (pos, cnt) in enumerate(ROWS):
        assert bool((bits[b, cnt:] == SENTINEL).all()), f"row {b}: a pad slot was written"
        if cnt == 0:
            continue
        qb, kb, vb = q[b:b + 1, :cnt], k[b:b + 1], v[b:b + 1]
        want, bound = ab.prefill_bound(qb, kb, vb, pos)
        ab.assert_attention_close(out[b:b + 1, :cnt], want, bound, f"G {G} row {b} (pos {pos}, count {cnt})")
        print(f"G {G} row {b} pos {pos} count {cnt}: worst error / bound {ab.worst_ratio(out[b:b + 1, :cnt], want, bound):.3f}")
        if pos + cnt > 1:   # the test must mean something: without its target row every query's reference moves > 100 bounds
            without, _ = ab.prefill_bound(qb, kb, vb, pos, drop=tgt[b])
            margin = ab.needle_margin(want, without, bound)[:, 1 if pos == 0 else 0:]
            assert float(margin.min()) > 100, (b, float(margin.min()))
        if pos > 0:
            assert (tgt[b] == pos - 1).any(), "a needle sits on the row just below the start"
            with pytest.raises(AssertionError):
                ab.assert_attention_close(shifted[b:b + 1, :cnt], want, bound, "wrong start")


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("mods", [False, True])
def test_equal_rows_are_the_shared_form_bit_for_bit(ops, G, mods):
    q, k, v, _ = _case(G)
    k, v = torch.nan_to_num(k, nan=0.25), torch.nan_to_num(v, nan=-0.5)
    B, Hq = q.shape[0], q.shape[2]
    kw = {}
    if mods:
        kw = dict(softcap=30.0, alibi_slopes=(0.5 ** torch.arange(1, Hq + 1, dtype=torch.float32)).cuda())
    want = ops.prefill_attention(q, k, v, 200, **kw)
    got = _run(ops, q, k, v, [200] * B, [S] * B, max_end=200 + S, **kw)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    got = _run(ops, q, k, v, [200] * B, [S] * B, max_end=TMAX, **kw)   # a looser host bound changes nothing
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_device_words_are_clamped_to_max_end(ops):
    """a count (or position) past the host's bound is cut to it: nothing at or above max_end is read, no slot behind the cut written"""
    q, k, v, _ = _case(1)
    pos, cnt = [0, 0, 127, 200, 383, 77], [1, 130, 2, 129, 400, 0]
    out = _run(ops, q, k, v, pos, cnt)
    want = _run(ops, q, k, v, [p for p, _ in ROWS], [c for _, c in ROWS])
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("G", [1, 4])
def test_append_with_counts(ops, kv8, G):
    from autoawq_amd.modules.fused.attn import RoPE

    Hq, B = HKV * G, len(ROWS)
    rope = RoPE(D, TMAX, "cuda", 10000.0)
    gen = torch.Generator().manual_seed(3 + G)
    qkv = torch.randn((B, S, (Hq + 2 * HKV) * D), generator=gen).half().cuda()
    pos, cnt = _i32([p for p, _ in ROWS]), _i32([c for _, c in ROWS])

    def caches():
        dt = torch.uint8 if kv8 else torch.float16
        kc, vc = _sentinel((B, TMAX, HKV, D), dt), _sentinel((B, TMAX, HKV, D), dt)
        sc = dict(k_scale=_sentinel((B, TMAX, HKV), torch.float32), v_scale=_sentinel((B, TMAX, HKV), torch.float32)) if kv8 else {}
        return kc, vc, sc

    kc, vc, sc = caches()
    q_n = ops.rope_kv_append(qkv, kc, vc, rope.cos, rope.sin, 0, Hq, HKV, D, D, pos_rows=pos, count_rows=cnt, **sc)
    # the plain rows form, one sequence at a time on its real slots only (as a batch its pad slots would spill over the rows)
    kr, vr, sr = caches()
    untouched = [x.clone() for x in (kr, vr) + tuple(sr.values())]
    for b, (p, c) in enumerate(ROWS):
        if c == 0:
            continue
        one = {n: t[b:b + 1] for n, t in sr.items()}
        q_r = ops.rope_kv_append(qkv[b:b + 1, :c].contiguous(), kr[b:b + 1], vr[b:b + 1], rope.cos, rope.sin, 0, Hq, HKV, D, D,
                                 pos_rows=pos[b:b + 1].contiguous(), **one)
        assert torch.equal(q_n[b, :c].view(torch.int16), q_r[0].view(torch.int16))
    got = (kc, vc) + tuple(sc.values())
    want = (kr, vr) + tuple(sr.values())
    for g, w, u in zip(got, want, untouched):
        as_bits = (lambda t: t.view(torch.int16)) if g.dtype == torch.float16 else (lambda t: t.view(torch.int32)) if g.dtype == torch.float32 else (lambda t: t)
        assert torch.equal(as_bits(g), as_bits(w))
        for b, (p, c) in enumerate(ROWS):   # and outside [pos, pos + count) nothing moved -- row TMAX - 1 of (383, 129) is real
            keep = torch.ones(TMAX, dtype=torch.bool, device="cuda")
            keep[p:p + c] = False
            assert torch.equal(as_bits(g[b][keep]), as_bits(u[b][keep])), b
            if c:
                assert not torch.equal(as_bits(g[b][p:p + c]), as_bits(u[b][p:p + c]))
    b = ROWS.index((383, 129))
    assert 383 + 129 == TMAX and not torch.equal(kc[b, TMAX - 1], untouched[0][b, TMAX - 1])


def test_refusals_match_the_shared_form(ops):
    from autoawq_amd import _lib

    L = _lib.lib()
    p, st = ops._ptr, ops._stream()
    B, Hq = 2, 4
    q = torch.zeros((B, 8, Hq, D), dtype=torch.float16, device="cuda")
    k = torch.zeros((B, 64, HKV, D), dtype=torch.float16, device="cuda")
    out = torch.zeros_like(q)
    pos, cnt = _i32([0, 0]), _i32([8, 8])

    def rows(q_=q, k_=k, out_=out, pos_=pos, cnt_=cnt, max_end=8, B_=B, S_=8, Hq_=Hq, Hkv_=HKV, D_=D, Tmax=64):
        return L.awq_prefill_attention_rows(p(q_), p(k_), p(k_), p(out_), p(pos_), p(cnt_), max_end, B_, S_, Hq_, Hkv_, D_, Tmax,
                                            1.0, 0.0, None, st)

    def shared(q_=q, k_=k, out_=out, B_=B, S_=8, Hq_=Hq, Hkv_=HKV, D_=D, Tmax=64, start=0):
        return L.awq_prefill_attention(p(q_), p(k_), p(k_), p(out_), B_, S_, Hq_, Hkv_, D_, Tmax, start, 1.0, 0.0, None, st)

    assert rows() == shared() == 0
    assert rows(D_=64) == shared(D_=64) == _lib.ERR_UNSUPPORTED
    assert rows(Hq_=3) == shared(Hq_=3) == _lib.ERR_UNSUPPORTED
    for kw in (dict(B_=-1), dict(Hkv_=0), dict(S_=-1)):
        assert rows(**kw) == shared(**kw) != 0
    assert rows(max_end=65) == shared(start=57) != 0                      # past the cache window
    off = torch.zeros(q.numel() + 8, dtype=torch.float16, device="cuda")[4:4 + q.numel()].view(q.shape)
    assert rows(q_=off) == shared(q_=off) != 0 and rows(out_=off) == shared(out_=off)   # alignment
    null = L.awq_prefill_attention_rows(p(q), p(k), p(k), None, p(pos), p(cnt), 8, B, 8, Hq, HKV, D, 64, 1.0, 0.0, None, st)
    assert null == L.awq_prefill_attention(p(q), p(k), p(k), None, B, 8, Hq, HKV, D, 64, 0, 1.0, 0.0, None, st) != 0
    assert L.awq_prefill_attention_rows(p(q), p(k), p(k), p(out), None, p(cnt), 8, B, 8, Hq, HKV, D, 64, 1.0, 0.0, None, st) == null
    # 32-bit offsets: 2^31 bytes of cache rows per sequence (refused on the host, nothing is launched)
    big = 1 << 22
    assert rows(max_end=big, Tmax=big) == shared(start=big - 8, Tmax=big) == _lib.ERR_UNSUPPORTED
    # the append: counts go with per-row positions, and the pointers are checked like the rows form's
    with pytest.raises(_lib.AwqHipError):
        ops.rope_kv_append(torch.zeros((B, 8, (Hq + 2 * HKV) * D), dtype=torch.float16, device="cuda"), k, k.clone(),
                           torch.zeros(64, 64, device="cuda"), torch.zeros(64, 64, device="cuda"), 0, Hq, HKV, D, D, count_rows=cnt)
    a = [None] * 8
    assert L.awq_rope_kv_append_rows_n(*a, B, 8, Hq, HKV, D, D, 64, st) == L.awq_rope_kv_append_rows(*a[:7], B, 8, Hq, HKV, D, D, 64, st) != 0
    a = [None] * 10
    assert (L.awq_rope_kv_append_rows_n_fp8(*a, B, 8, Hq, HKV, D, D, 64, st)
            == L.awq_rope_kv_append_rows_fp8(*a[:9], B, 8, Hq, HKV, D, D, 64, st) != 0)
