"""awq_verify_attention_rows (csrc/verify_attn.hip) against the fp64 reference of tests/attn_bound.py, within the decode-class bound
(tests/spec_attn_bound.py: nothing in the arithmetic differs, only the split count).  Every G x T, contexts on both sides of the
one-split limit (256 rows) and of a 16-row chunk edge, different positions in one launch including 0, a short row in a long
bucket, cache rows above pos_b + T - 1 filled with NaN.  Needles: for every (b, j) the newest row that pair may see, pos_b + j,
carries nearly all of its softmax weight and must show in the output; an anti-needle at pos_b + j + 1 must not."""
import pytest
import torch

import attn_bound as ab
import attn_needles as nd
import spec_attn_bound as sb

pytestmark = pytest.mark.gpu
D = 128


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import ops as o

    return o


def _launch(ops, q, k, v, pos, max_len):
    p = torch.tensor(pos, dtype=torch.int32).cuda()
    return ops.verify_attention_rows(q.cuda(), k.cuda().contiguous(), v.cuda().contiguous(), p, max_len=max_len).cpu()


def _poison(k, v, pos, T):
    for b, p in enumerate(pos):
        k[b, p + T:] = float("nan")
        v[b, p + T:] = float("nan")


# (positions of the sequences, max_len or None = the cache window): both sides of 256 rows, of a 16-row chunk edge, pos 0,
# a short row in a long bucket
def _cases(T):
    return [([0, 5, 16 - T, 17 - T], 64, 64),          # one split; pos_b + T on both sides of a 16-row edge
            ([256 - T, 0, 100], 256, 256),             # exactly the one-split limit
            ([257 - T, 1, 255 - T], 300, 300),         # just past it: 3 splits, chunk edges inside the new rows' neighbourhood
            ([1000, 3, 0, 511], 2048, 2048),           # short rows in a long bucket: empty splits
            ([700 - T, 690], 1024, 704)]               # max_len below the window; pos_b + T = 700 .. 698


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("T", [2, 3, 4, 8])
def test_verify_attention_random(ops, G, T):
    from autoawq_amd import ops as O

    worst = 0.0
    for ci, (pos, Tmax, max_len) in enumerate(_cases(T)):
        B, Hkv = len(pos), 2
        Hq = Hkv * G
        gen = torch.Generator().manual_seed(1000 * G + 10 * T + ci)
        q = torch.randn((B, T, Hq, D), generator=gen).half()
        k = torch.randn((B, Tmax, Hkv, D), generator=gen).half()
        v = torch.randn((B, Tmax, Hkv, D), generator=gen).half()
        _poison(k, v, pos, T)
        splits = sb.verify_splits(max_len, B, T, Hq, Hkv)
        assert splits == O.verify_attention_splits(max_len, B, T, Hq, Hkv)
        out = _launch(ops, q, k, v, pos, max_len)
        want, bound = sb.verify_bound(q.cuda(), k.cuda(), v.cuda(), pos, splits)
        what = f"G {G} T {T} pos {pos} max_len {max_len} splits {splits}"
        ab.assert_attention_close(out.cuda(), want, bound, what)
        worst = max(worst, ab.worst_ratio(out.cuda(), want, bound))
    print(f"worst error / bound G {G} T {T}: {worst:.3f}")


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("T", [2, 3, 4, 8])
@pytest.mark.parametrize("parity", [0, 1])
def test_verify_attention_needles(ops, G, T, parity):
    """Query (b, j) is c * the key of row pos_b + j.  For j = parity mod 2 (j < T - 1) the key of row pos_b + j + 1 is TWICE the
    key of row pos_b + j: it would outscore the target if query j saw it, is legitimate for query j + 1 (whose target it is), and is
    invisible to query j."""
    worst = 0.0
    for ci, (pos, Tmax, max_len) in enumerate(_cases(T)):
        B, Hkv = len(pos), 2
        Hq = Hkv * G
        gen = torch.Generator().manual_seed(77 + 1000 * G + 10 * T + ci)
        k = nd.pm1(gen, (B, Tmax, Hkv, D))
        v = torch.randn((B, Tmax, Hkv, D), generator=gen).half()
        anti = torch.zeros((B, T), dtype=torch.bool)
        for b, p in enumerate(pos):
            for j in range(parity, T - 1, 2):
                k[b, p + j + 1] = k[b, p + j] * 2
                anti[b, j] = True
        q = torch.empty((B, T, Hq, D), dtype=torch.float16)
        tgt = torch.empty((B, T, Hq), dtype=torch.int64)
        for b, p in enumerate(pos):
            for j in range(T):
                tgt[b, j] = p + j
                for h in range(Hq):
                    q[b, j, h] = (2.0 * k[b, p + j, h // G].float()).half()
        _poison(k, v, pos, T)
        splits = sb.verify_splits(max_len, B, T, Hq, Hkv)
        out = _launch(ops, q, k, v, pos, max_len)
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
        want, bound = sb.verify_bound(qd, kd, vd, pos, splits)
        what = f"needles G {G} T {T} parity {parity} pos {pos} splits {splits}"
        ab.assert_attention_close(out.cuda(), want, bound, what)
        worst = max(worst, ab.worst_ratio(out.cuda(), want, bound))
        # the needle must show: without its target row every (b, j, h) with more than one visible row moves > 100 bounds
        vis = sb.verify_pos(pos, T, Tmax)
        without = ab.reference(qd, kd, vd, vis, drop=tgt)["out"]
        margin = ab.needle_margin(want, without, bound).cpu()
        live = (vis > 0).view(B, T, 1).expand(B, T, Hq)
        assert bool((margin[live] > 100).all()), (what, float(margin[live].min()))
        # the anti-needle must NOT show: had query j seen row pos_b + j + 1, its output would lie > 100 bounds away
        if bool(anti.any()):
            seen = ab.reference(qd, kd, vd, vis + anti.to(torch.int64))["out"]
            am = ab.needle_margin(want, seen, bound).cpu()
            sel = anti.view(B, T, 1).expand(B, T, Hq)
            assert bool((am[sel] > 100).all()), (what, float(am[sel].min()))
    print(f"worst error / bound needles G {G} T {T} parity {parity}: {worst:.3f}")


def test_verify_attention_refusals(ops):
    from autoawq_amd import _lib

    k = torch.zeros((1, 32, 1, D), dtype=torch.float16, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    for T, Hq in ((1, 1), (9, 1), (2, 3)):
        q = torch.zeros((1, T, Hq, D), dtype=torch.float16, device="cuda")
        kk = k if Hq != 3 else k
        with pytest.raises(_lib.AwqHipError) as e:
            ops.verify_attention_rows(q, kk, kk.clone(), pos)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    q = torch.zeros((1, 2, 1, D), dtype=torch.float16, device="cuda")
    with pytest.raises(NotImplementedError, match="fp8"):
        ops.verify_attention_rows(q, k.to(torch.uint8), k.to(torch.uint8), pos)
    # a device-side position past the cache is clamped like the append's: the last row, never memory behind the cache
    big = torch.full((1,), 1 << 20, dtype=torch.int32, device="cuda")
    kc = torch.randn((1, 32, 1, D), device="cuda").half()
    out = ops.verify_attention_rows(torch.randn((1, 2, 1, D), device="cuda").half(), kc, kc.clone(), big)
    assert bool(torch.isfinite(out).all())
