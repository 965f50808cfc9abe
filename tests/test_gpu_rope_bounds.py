"""RoPE + KV append, every form, against the float64 rotation and its window (tests/norm_rope_bound.py): the six append entry
points on Gaussian rows, rows built to cancel (a cos ~ b sin), rows that overflow fp16, subnormals, +-0 and NaN; NaN payloads,
infinities and -0 in the dims and rows that are only copied, compared as bits; and the WHOLE cache compared with its expected
image, sentinel included.  The fp16 forms are held to the window; the fp8 forms to the quantisation (tests/kv8_ref.py) of what the
fp16 form wrote; the fused decode step to the caches the append kernel leaves, bit for bit, on the rows where the three ways of
contracting a * c - b * s into an fma differ most.  Every device position lies inside its cache.

NORM_ROPE_BOUND_RECORD=<file>: every case appends "implementation shape kind eps ratio" (recorded, not asserted)."""
import numpy as np
import pytest
import torch

import kv8_ref
import norm_rope_bound as nrb

pytestmark = pytest.mark.gpu

ENTRIES = ("start_pos", "pos_dev", "pos_rows", "count_rows")  # awq_rope_kv_append (host word, device word), _rows, _rows_n


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(v):
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device="cuda")


_tables, _sentinels = {}, {}


def tables(rot, Tmax, theta):
    """(cos, sin) numpy and on the device; rot == 0 hands the kernel a one-column table it never reads"""
    key = (rot, Tmax, theta)
    if key not in _tables:
        cos, sin = nrb.rope_tables(rot, Tmax, theta)
        pad = np.zeros((Tmax, 1), np.float32)
        _tables[key] = (cos, sin, dev(cos if rot else pad), dev(sin if rot else pad))
    return _tables[key]


def sentinel(B, Tmax, Hkv, D):
    """the caches before the call: (k, v) fp16 numpy, their device copies, and their fp8 form (D = 128) -- made once per shape"""
    key = (B, Tmax, Hkv, D)
    if key not in _sentinels:
        rng = np.random.default_rng([B, Tmax, Hkv, D])
        k, v = rng.standard_normal((B, Tmax, Hkv, D)).astype(np.float16), rng.standard_normal((B, Tmax, Hkv, D)).astype(np.float16)
        e = {"k": k, "v": v, "kd": dev(k), "vd": dev(v)}
        if D == 128:
            for n in ("k", "v"):
                codes, scales = kv8_ref.quantize(e[n])
                e[n + "c"], e[n + "s"], e[n + "cd"], e[n + "sd"] = codes, scales, dev(codes), dev(scales)
        _sentinels[key] = e
    return _sentinels[key]


def append(ops, entry, qkv, kc, vc, cos_d, sin_d, pos, prow, counts, Hq, Hkv, D, rot, **scales):
    if entry == "start_pos":
        return ops.rope_kv_append(qkv, kc, vc, cos_d, sin_d, pos, Hq, Hkv, D, rot, **scales)
    if entry == "pos_dev":
        return ops.rope_kv_append(qkv, kc, vc, cos_d, sin_d, 0, Hq, Hkv, D, rot, pos_dev=i32([pos]), **scales)
    if entry == "pos_rows":
        return ops.rope_kv_append(qkv, kc, vc, cos_d, sin_d, 0, Hq, Hkv, D, rot, pos_rows=i32(prow), **scales)
    return ops.rope_kv_append(qkv, kc, vc, cos_d, sin_d, 0, Hq, Hkv, D, rot, pos_rows=i32(prow), count_rows=i32(counts), **scales)


def layout(entry, case):
    """(positions [B], counts [B] or None) of a case under an entry point: the shared forms put every sequence at `pos`"""
    _, _, B, S, _, Tmax, pos, _, counts = case
    prow = nrb.row_positions(pos, B, S, Tmax) if entry in ("pos_rows", "count_rows") else [pos] * B
    assert all(0 <= p and p + S <= Tmax for p in prow)  # every device word inside the cache
    return prow, (counts if entry == "count_rows" else None)


def live_slots(B, S, cnt):
    return np.array([[cnt is None or s < cnt[b] for s in range(S)] for b in range(B)])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("D,rot", nrb.ROPE_DIMS)
def test_rope_kv_append_window(ops, D, rot, entry):
    for case in nrb.rope_cases(D, rot):
        Hq, Hkv, B, S, theta, Tmax, pos, kind, _ = case
        cos, sin, cos_d, sin_d = tables(rot, Tmax, theta)
        prow, cnt = layout(entry, case)
        qkv = nrb.rope_rows(kind, B, S, Hq, Hkv, D, rot, cos, sin, prow, seed=5)
        x = qkv.reshape(B, S, Hq + 2 * Hkv, D)
        P = (np.asarray(prow)[:, None] + np.arange(S)[None, :])[:, :, None]
        st = sentinel(B, Tmax, Hkv, D)
        kc, vc = st["kd"].clone(), st["vd"].clone()
        q = append(ops, entry, dev(qkv), kc, vc, cos_d, sin_d, pos, prow, cnt, Hq, Hkv, D, rot).cpu().numpy()
        what = f"{entry} D{D} rot{rot} {case}"
        live = live_slots(B, S, cnt)
        lo, hi, exact = nrb.rope_window(x[:, :, :Hq], cos, sin, P, rot)
        nrb.assert_rows_in_window(q[live], lo[live], hi[live], exact[live], "q " + what)   # (q of a slot past its count is unspecified)
        klo, khi, kex = nrb.rope_window(x[:, :, Hq:Hq + Hkv], cos, sin, P, rot)
        kgot = kc.cpu().numpy()
        nrb.assert_rows_in_window(kgot, nrb.cache_image(st["k"], klo, prow, cnt), nrb.cache_image(st["k"], khi, prow, cnt),
                                  nrb.cache_image(np.ones(st["k"].shape, bool), kex, prow, cnt), "k cache " + what)
        vimg = nrb.cache_image(st["v"], x[:, :, Hq + Hkv:], prow, cnt)
        assert np.array_equal(vc.cpu().numpy().view(np.uint16), vimg.view(np.uint16)), "v cache " + what
        krows = np.stack([kgot[b, prow[b]:prow[b] + S] for b in range(B)])
        ratio = max(nrb.rope_ratio(q[live], x[:, :, :Hq][live], cos, sin, P[live], rot),
                    nrb.rope_ratio(krows[live], x[:, :, Hq:Hq + Hkv][live], cos, sin, P[live], rot)) if live.any() else 0.0
        nrb.record(f"rope_kv_append[{entry}]", f"D{D} rot{rot} Hq{Hq} Hkv{Hkv} B{B} S{S} theta{theta:g} pos{pos}", kind, 0.0, ratio)


def quantized_image(st, n, cache16, prow, S, cnt):
    """kv8_ref.quantize of the whole fp16 cache: the format is row by row, so it is the sentinel's codes and scales (made once)
    with the rows the fp16 form wrote quantised in their places -- after checking that the fp16 form left the rest alone"""
    B = len(prow)
    rows = np.stack([cache16[b, prow[b]:prow[b] + S] for b in range(B)])
    assert np.array_equal(nrb.cache_image(cache16, st[n][:B, :S], prow, cnt).view(np.uint16),
                          nrb.cache_image(st[n], st[n][:B, :S], prow, cnt).view(np.uint16))
    codes, scales = kv8_ref.quantize(rows)
    return nrb.cache_image(st[n + "c"], codes, prow, cnt), nrb.cache_image(st[n + "s"], scales, prow, cnt)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("rot", [128, 64, 0])
def test_rope_kv_append_fp8_is_the_quantised_fp16_form(ops, rot, entry):
    D = 128
    for case in nrb.rope_cases(D, rot):
        Hq, Hkv, B, S, theta, Tmax, pos, kind, _ = case
        cos, sin, cos_d, sin_d = tables(rot, Tmax, theta)
        prow, cnt = layout(entry, case)
        qkv = dev(nrb.rope_rows(kind, B, S, Hq, Hkv, D, rot, cos, sin, prow, seed=5))
        st = sentinel(B, Tmax, Hkv, D)
        k16, v16 = st["kd"].clone(), st["vd"].clone()
        q16 = append(ops, entry, qkv, k16, v16, cos_d, sin_d, pos, prow, cnt, Hq, Hkv, D, rot)
        kc, vc, ks, vs = st["kcd"].clone(), st["vcd"].clone(), st["ksd"].clone(), st["vsd"].clone()
        q8 = append(ops, entry, qkv, kc, vc, cos_d, sin_d, pos, prow, cnt, Hq, Hkv, D, rot, k_scale=ks, v_scale=vs)
        what = f"{entry} rot{rot} {case}"
        live = torch.from_numpy(live_slots(B, S, cnt)).cuda()
        assert torch.equal(q8.view(torch.int16)[live], q16.view(torch.int16)[live]), "q " + what
        for n, c16, codes, scales in (("k", k16, kc, ks), ("v", v16, vc, vs)):
            want_c, want_s = quantized_image(st, n, c16.cpu().numpy(), prow, S, cnt)
            assert np.array_equal(codes.cpu().numpy(), want_c), f"{n} codes {what}"
            assert np.array_equal(scales.cpu().numpy(), want_s, equal_nan=True), f"{n} scales {what}"


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("rows", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("kv8", [False, True], ids=["fp16", "fp8"])
def test_fused_step_appends_the_rows_of_the_append_kernel(ops, kv8, rows, G):
    """awq_decode_attention_rope leaves the caches rope_kv_append leaves, bit for bit, on rows where the fma contractions of the
    rotation differ (`cancel`), overflow (`big`) or underflow; only the caches are asserted here -- the attention output of
    Gaussian rows keeps its bound tests (test_gpu_attention_bounds.py, test_decoder.py)"""
    Hkv, D, Tmax = 2, 128, nrb.FUSED_TMAX
    Hq, B = Hkv * G, 3 if rows else 2
    st = sentinel(B, Tmax, Hkv, D)
    names = ("kcd", "vcd", "ksd", "vsd") if kv8 else ("kd", "vd")
    for i, pos in enumerate(nrb.FUSED_POSITIONS):
        cos, sin, cos_d, sin_d = tables(D, Tmax, nrb.ROPE_THETAS[i])
        prow = nrb.row_positions(pos, B, 1, Tmax) if rows else [pos] * B
        assert all(0 <= p < Tmax for p in prow)
        for kind in nrb.FUSED_KINDS:
            qkv = dev(nrb.rope_rows(kind, B, 1, Hq, Hkv, D, D, cos, sin, prow, seed=5))
            a = [st[n].clone() for n in names]
            sc = dict(k_scale=a[2], v_scale=a[3]) if kv8 else {}
            append(ops, "pos_rows" if rows else "start_pos", qkv, a[0], a[1], cos_d, sin_d, pos, prow, None, Hq, Hkv, D, D, **sc)
            for use_dev in ((False,) if rows else (False, True)):
                f = [st[n].clone() for n in names]
                sc = dict(k_scale=f[2], v_scale=f[3]) if kv8 else {}
                if rows:
                    ops.decode_attention_rope(qkv, f[0], f[1], cos_d, sin_d, 0, Hq, Hkv, pos_rows=i32(prow), max_len=Tmax, **sc)
                elif use_dev:
                    ops.decode_attention_rope(qkv, f[0], f[1], cos_d, sin_d, 0, Hq, Hkv, pos_dev=i32([pos]), max_len=Tmax, **sc)
                else:
                    ops.decode_attention_rope(qkv, f[0], f[1], cos_d, sin_d, pos, Hq, Hkv, **sc)
                for n, got, want in zip(names, f, a):
                    as_int = {torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[got.dtype]
                    same = got.view(as_int) == want.view(as_int)
                    assert bool(same.all()), (f"{n} differs from the append kernel's in {int((~same).sum())} elements: {kind} pos {pos} "
                                              f"G{G} device word {use_dev}; first at {[int(v) for v in (~same).nonzero()[0]]}")
