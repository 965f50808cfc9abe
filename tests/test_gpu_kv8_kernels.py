"""fp8 KV cache kernels on the MI355X: conversions, append, decode attention (every G and form) against the oracle on the
dequantized cache, self-consistency (fused == append + plain, rows == alone, graph == eager), NaN rows, prefill workspace."""
import numpy as np
import pytest
import torch

import attn_bound
import kv8_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import ops as o

    return o


def _cache(B, T, H, gen, scale=1.0):
    x = (torch.randn((B, T, H, 128), generator=gen) * scale).half()
    codes, s = ref.quantize(x.numpy())
    return x, torch.from_numpy(codes).cuda(), torch.from_numpy(s).cuda()


def test_decode_all_256_codes(ops):
    codes = torch.arange(256, dtype=torch.uint8).view(1, 2, 1, 128).cuda()
    s = torch.ones((1, 2, 1), dtype=torch.float32, device="cuda")
    got = ops.kv_dequant_fp8(codes, s, 2).float().cpu().view(-1).numpy()
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().half().float().numpy()
    assert np.array_equal(got, want, equal_nan=True)


def test_encode_tie_points_round_to_even(ops):
    t = ref.decode_table()[:127]
    mids = (t[:-1] + t[1:]) / 2                          # every tie between two neighbouring non-negative codes
    vals = np.concatenate([mids, -mids, t, -t])
    vals = vals[np.abs(vals) <= 448.0]
    n = (len(vals) + 126) // 127
    rows = np.zeros((n, 128))
    rows[:, 0] = 448.0                                   # amax 448: scale 1, the values are coded as they are
    rows[:, 1:].reshape(-1)[: len(vals)] = vals
    x16 = rows.astype(np.float16)
    assert np.array_equal(x16.astype(np.float64), rows)  # all ties exactly representable in fp16
    cache = torch.zeros((1, n, 1, 128), dtype=torch.uint8, device="cuda")
    sc = torch.zeros((1, n, 1), dtype=torch.float32, device="cuda")
    ops.kv_quant_fp8(torch.from_numpy(x16).view(1, n, 1, 128).cuda(), cache, sc)
    want_c, want_s = ref.quantize(x16)
    assert np.array_equal(sc.cpu().view(-1).numpy(), want_s)
    assert np.array_equal(cache.cpu().view(n, 128).numpy(), want_c)
    torch_c = torch.from_numpy(rows).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(want_c, torch_c)


def test_quant_dequant_special_rows(ops):
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn((1, 8, 2, 128), generator=gen) * torch.tensor([1e-6, 1e-3, 1.0, 300.0, 6e4, 1.0, 1.0, 1.0]).view(1, 8, 1, 1)).half()
    x[0, 5, 0] = 0
    x[0, 6, 1, 3] = float("nan")
    x[0, 7, 0, 9] = float("-inf")
    x[0, 4, 1, 0] = 65504.0
    cache = torch.zeros((1, 8, 2, 128), dtype=torch.uint8, device="cuda")
    sc = torch.zeros((1, 8, 2), dtype=torch.float32, device="cuda")
    ops.kv_quant_fp8(x.cuda(), cache, sc)
    wc, ws = ref.quantize(x.numpy())
    assert np.array_equal(cache.cpu().numpy(), wc) and np.array_equal(sc.cpu().numpy(), ws, equal_nan=True)
    back = ops.kv_dequant_fp8(cache, sc, 8).cpu().numpy()
    assert np.array_equal(back, ref.dequantize_fp16(wc, ws), equal_nan=True)


def _rope(Tmax):
    from autoawq_amd.modules.fused.attn import RoPE

    r = RoPE(128, Tmax, "cuda", 10000)
    return r.cos, r.sin


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("rot", [128, 64])
def test_append_matches_restatement_of_fp16_append(ops, rows, rot):
    B, S, Hq, Hkv, Tmax = 3, 5, 8, 2, 32
    gen = torch.Generator().manual_seed(11 + rot + rows)
    qkv = (torch.randn((B, S, (Hq + 2 * Hkv) * 128), generator=gen) * 4).half().cuda()
    qkv[1, 2, (Hq + 1) * 128 + 7] = float("nan")  # one k row of sequence 1 holds a NaN
    qkv[2, 0, (Hq + Hkv) * 128:] = 0              # v rows of zeros
    cos, sin = _rope(Tmax)
    kc = torch.zeros((B, Tmax, Hkv, 128), dtype=torch.float16, device="cuda")
    vc = torch.zeros_like(kc)
    k8 = torch.zeros((B, Tmax, Hkv, 128), dtype=torch.uint8, device="cuda")
    v8 = torch.zeros_like(k8)
    ks = torch.zeros((B, Tmax, Hkv), dtype=torch.float32, device="cuda")
    vs = torch.zeros_like(ks)
    pos = torch.tensor([3, 9, 0], dtype=torch.int32, device="cuda") if rows else None
    q16 = ops.rope_kv_append(qkv, kc, vc, cos, sin, 4, Hq, Hkv, 128, rot, pos_rows=pos)
    q8 = ops.rope_kv_append(qkv, k8, v8, cos, sin, 4, Hq, Hkv, 128, rot, pos_rows=pos, k_scale=ks, v_scale=vs)
    assert torch.equal(q16, q8)
    for c16, c8, s8 in ((kc, k8, ks), (vc, v8, vs)):
        wc, wsc = ref.quantize(c16.cpu().numpy())
        assert np.array_equal(c8.cpu().numpy(), wc)
        assert np.array_equal(s8.cpu().numpy(), wsc, equal_nan=True)
    assert torch.isnan(ks).any()


FORMS = ["plain", "fused", "extra", "rows", "rows_extra", "fused_rows"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_decode_attention_vs_oracle(ops, G, form):
    """Every form against the oracle on the dequantized cache.  Rows at or past each sequence's length are poisoned (NaN scales,
    codes of 448): a kernel that used one of them would return NaN.  The *rows forms give the two sequences different lengths."""
    from oracle import decoder_oracle

    B, Hkv = 2, 2
    Hq = G * Hkv
    rows = form.startswith("rows") or form == "fused_rows"
    for T in (1, 17, 256, 1000, 4096):
        gen = torch.Generator().manual_seed(G * 1000 + T + FORMS.index(form))
        Tmax = T + 8
        lens = [T, max(1, (T + 1) // 3)] if rows else [T, T]
        _, k8, ks = _cache(B, Tmax, Hkv, gen)
        _, v8, vs = _cache(B, Tmax, Hkv, gen, 0.5)
        for b, L in enumerate(lens):
            for c8, sc in ((k8, ks), (v8, vs)):
                c8[b, L:] = 0x7E
                sc[b, L:] = float("nan")
        q = torch.randn((B, Hq, 128), generator=gen).half()
        softcap, slopes = (20.0, decoder_oracle.alibi_slopes_reference(Hq)) if form.endswith("extra") else (0.0, None)
        sl = torch.from_numpy(slopes).float().cuda() if slopes is not None else None
        ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
        if form.startswith("fused"):
            cos, sin = _rope(Tmax)
            qkv = (torch.randn((B, 1, (Hq + 2 * Hkv) * 128), generator=gen)).half().cuda()
            pos = (ln - 1).contiguous()
            if rows:
                out = ops.decode_attention_rope(qkv, k8, v8, cos, sin, 0, Hq, Hkv, pos_rows=pos, max_len=Tmax, k_scale=ks,
                                                v_scale=vs)
            else:
                out = ops.decode_attention_rope(qkv, k8, v8, cos, sin, T - 1, Hq, Hkv, k_scale=ks, v_scale=vs)
            # the oracle runs on what the step appended: the rotated q comes from the fp16 append of the same row
            z = torch.zeros((B, Tmax, Hkv, 128), dtype=torch.float16, device="cuda")
            q = ops.rope_kv_append(qkv, z, z.clone(), cos, sin, T - 1, Hq, Hkv, 128, 128, pos_rows=pos if rows else None)[:, 0].cpu()
        elif rows:
            out = ops.decode_attention(q.cuda(), k8, v8, 1, len_rows=ln, max_len=Tmax, softcap=softcap, alibi_slopes=sl,
                                       k_scale=ks, v_scale=vs)
        else:
            out = ops.decode_attention(q.cuda(), k8, v8, T, softcap=softcap, alibi_slopes=sl, k_scale=ks, v_scale=vs)
        kd = ref.dequantize(k8.cpu().numpy(), ks.cpu().numpy())
        vd = ref.dequantize(v8.cpu().numpy(), vs.cpu().numpy())
        got = out.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any(), (G, form, T, "a poisoned row was read")
        for b, L in enumerate(lens):
            want = decoder_oracle.attention_reference(q.numpy()[b:b + 1], kd[b:b + 1], vd[b:b + 1], L, softcap=softcap,
                                                      alibi_slopes=slopes)
            assert np.abs(got[b:b + 1] - want).max() <= 2e-3 * np.abs(want).max() + 2 ** -11, (G, form, T, b)
        # the derived per-element bound (tests/attn_bound.py) on the dequantised cache, split count of the launch
        splits = attn_bound.decode_splits(Tmax if rows else T, B, Hq, Hkv)
        w, bound = attn_bound.decode_bound(q, torch.from_numpy(kd), torch.from_numpy(vd), lens, splits, softcap=softcap,
                                           alibi=None if slopes is None else torch.from_numpy(slopes).float())
        attn_bound.assert_attention_close(torch.from_numpy(got), w, bound, f"{form} G {G} T {T}")


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_fused_equals_append_then_plain(ops, G):
    B, Hkv = 2, 2
    Hq = G * Hkv
    for T in (1, 40, 700):
        gen = torch.Generator().manual_seed(G + T)
        Tmax = T + 4
        cos, sin = _rope(Tmax)
        _, k8, ks = _cache(B, Tmax, Hkv, gen)
        _, v8, vs = _cache(B, Tmax, Hkv, gen)
        k8b, v8b, ksb, vsb = k8.clone(), v8.clone(), ks.clone(), vs.clone()
        qkv = torch.randn((B, 1, (Hq + 2 * Hkv) * 128), generator=gen).half().cuda()
        fused = ops.decode_attention_rope(qkv, k8, v8, cos, sin, T - 1, Hq, Hkv, k_scale=ks, v_scale=vs)
        q = ops.rope_kv_append(qkv, k8b, v8b, cos, sin, T - 1, Hq, Hkv, 128, 128, k_scale=ksb, v_scale=vsb)
        plain = ops.decode_attention(q[:, 0], k8b, v8b, T, k_scale=ksb, v_scale=vsb)
        assert torch.equal(k8, k8b) and torch.equal(v8, v8b) and torch.equal(ks, ksb) and torch.equal(vs, vsb)
        assert torch.equal(fused, plain), (G, T)


def test_rows_equal_each_row_alone(ops):
    B, Hq, Hkv, Tmax = 3, 8, 2, 600
    gen = torch.Generator().manual_seed(21)
    _, k8, ks = _cache(B, Tmax, Hkv, gen)
    _, v8, vs = _cache(B, Tmax, Hkv, gen)
    q = torch.randn((B, Hq, 128), generator=gen).half().cuda()
    lens = [5, 300, 577]
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    got = ops.decode_attention(q, k8, v8, 1, len_rows=ln, max_len=Tmax, k_scale=ks, v_scale=vs)
    for b, L in enumerate(lens):
        one = torch.tensor([L], dtype=torch.int32, device="cuda")
        alone = ops.decode_attention(q[b:b + 1].contiguous(), k8[b:b + 1].contiguous(), v8[b:b + 1].contiguous(), 1, len_rows=one,
                                     max_len=Tmax, k_scale=ks[b:b + 1].contiguous(), v_scale=vs[b:b + 1].contiguous())
        assert torch.equal(got[b:b + 1], alone), b
    cos, sin = _rope(Tmax)
    qkv = torch.randn((B, 1, (Hq + 2 * Hkv) * 128), generator=gen).half().cuda()
    pos = torch.tensor([4, 299, 576], dtype=torch.int32, device="cuda")
    k2, v2, ks2, vs2 = k8.clone(), v8.clone(), ks.clone(), vs.clone()
    fused = ops.decode_attention_rope(qkv, k2, v2, cos, sin, 0, Hq, Hkv, pos_rows=pos, max_len=Tmax, k_scale=ks2, v_scale=vs2)
    for b in range(B):
        kk, vv, kss, vss = (t[b:b + 1].clone() for t in (k8, v8, ks, vs))
        p = pos[b:b + 1].contiguous()
        alone = ops.decode_attention_rope(qkv[b:b + 1].contiguous(), kk, vv, cos, sin, 0, Hq, Hkv, pos_rows=p, max_len=Tmax,
                                          k_scale=kss, v_scale=vss)
        assert torch.equal(fused[b:b + 1], alone) and torch.equal(k2[b:b + 1], kk) and torch.equal(ks2[b:b + 1], kss)


def test_graph_replay_equals_eager(ops):
    B, Hq, Hkv, Tmax = 2, 8, 2, 512
    gen = torch.Generator().manual_seed(31)
    _, k8, ks = _cache(B, Tmax, Hkv, gen)
    _, v8, vs = _cache(B, Tmax, Hkv, gen)
    cos, sin = _rope(Tmax)
    qkv = torch.randn((B, 1, (Hq + 2 * Hkv) * 128), generator=gen).half().cuda()
    pos = torch.tensor([300], dtype=torch.int32, device="cuda")
    k2, v2, ks2, vs2 = k8.clone(), v8.clone(), ks.clone(), vs.clone()
    eager = ops.decode_attention_rope(qkv, k2, v2, cos, sin, 0, Hq, Hkv, pos_dev=pos, max_len=Tmax, k_scale=ks2, v_scale=vs2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.decode_attention_rope(qkv, k8.clone(), v8.clone(), cos, sin, 0, Hq, Hkv, pos_dev=pos, max_len=Tmax, k_scale=ks.clone(),
                                  v_scale=vs.clone())  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.decode_attention_rope(qkv, k8, v8, cos, sin, 0, Hq, Hkv, pos_dev=pos, max_len=Tmax, k_scale=ks, v_scale=vs)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(k8, k2) and torch.equal(ks, ks2)


@pytest.mark.parametrize("T", [40, 600])  # one split; several splits (the partials and the combine kernel carry the NaN)
def test_nan_row_gives_nan(ops, T):
    B, Hq, Hkv = 1, 4, 2
    gen = torch.Generator().manual_seed(41)
    x, k8, ks = _cache(B, T, Hkv, gen)
    _, v8, vs = _cache(B, T, Hkv, gen)
    ks[0, 13, 1] = float("nan")
    q = torch.randn((B, Hq, 128), generator=gen).half().cuda()
    out = ops.decode_attention(q, k8, v8, T, k_scale=ks, v_scale=vs).cpu()
    assert torch.isnan(out[0, 2:]).all() and not torch.isnan(out[0, :2]).any()  # heads 2, 3 read KV head 1


@pytest.mark.parametrize("start", [0, 37])
def test_prefill_on_dequantized_rows(ops, start):
    B, S, Hq, Hkv, Tmax = 2, 50, 8, 2, 128
    gen = torch.Generator().manual_seed(51 + start)
    cos, sin = _rope(Tmax)
    x, k8, ks = _cache(B, Tmax, Hkv, gen)
    _, v8, vs = _cache(B, Tmax, Hkv, gen)
    qkv = torch.randn((B, S, (Hq + 2 * Hkv) * 128), generator=gen).half().cuda()
    q = ops.rope_kv_append(qkv, k8, v8, cos, sin, start, Hq, Hkv, 128, 128, k_scale=ks, v_scale=vs)
    kw = ops.kv_dequant_fp8(k8, ks, start + S)
    vw = ops.kv_dequant_fp8(v8, vs, start + S)
    assert np.array_equal(kw.cpu().numpy(), ref.dequantize_fp16(k8[:, :start + S].cpu().numpy(), ks[:, :start + S].cpu().numpy()))
    got = ops.prefill_attention(q, kw, vw, start)
    k16 = torch.zeros((B, Tmax, Hkv, 128), dtype=torch.float16)
    v16 = torch.zeros_like(k16)
    k16[:, :start + S] = torch.from_numpy(ref.dequantize_fp16(k8[:, :start + S].cpu().numpy(), ks[:, :start + S].cpu().numpy()))
    v16[:, :start + S] = torch.from_numpy(ref.dequantize_fp16(v8[:, :start + S].cpu().numpy(), vs[:, :start + S].cpu().numpy()))
    want = ops.prefill_attention(q, k16.cuda(), v16.cuda(), start)
    assert torch.equal(got, want)
