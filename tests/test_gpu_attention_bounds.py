"""Attention kernels against the fp64 reference within the derived per-element bound (tests/attn_bound.py), on inputs where every
row and every split is visible (tests/attn_needles.py): each query head targets one row -- the early-prefetch set, every split
boundary of the launch, the last row, the fused forms' new token, each sequence's own last row -- so that a row lost or counted
twice moves that head's output by O(1), far outside the bound (checked: the reference without the target row lies > 100 bounds
away).  Also: split counts only the C ABI's workspace limit produces, scores over the whole fp32 exp range, and needle prefill
with anti-needles just past the causal diagonal."""
import pytest
import torch

import attn_bound as ab
import attn_needles as nd
import kv8_ref

pytestmark = pytest.mark.gpu

D = 128
C = 2.0
FORMS = ["plain", "extra", "rows", "rows_extra", "fused", "fused_rows"]
LENGTHS = [1, 16, 64, 65, 256, 257, 1000, 4096]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()
    return _ops


def _rope(Tmax):
    from autoawq_amd.modules.fused.attn import RoPE

    r = RoPE(128, Tmax, "cuda", 10000.0)
    return r.cos, r.sin


_TABLE = {}


def dequant(codes, scales):
    """kv8_ref.dequantize on the device: code * scale in float64"""
    dev = codes.device
    if dev not in _TABLE:
        _TABLE[dev] = torch.from_numpy(kv8_ref.decode_table()).to(dev)
    return _TABLE[dev][codes.long()] * scales.double()[..., None]


def quant(x):
    """fp16 rows -> fp8 cache codes and scales (awq_kv_quant_fp8, on the device; the reference reads back what it wrote)"""
    from autoawq_amd import ops

    x = x.cuda()
    codes = torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    scales = torch.empty(x.shape[:3], dtype=torch.float32, device="cuda")
    ops.kv_quant_fp8(x, codes, scales)
    return codes, scales


def deal_distinct(rows_per_seq, B, Hkv, G, it):
    """[B, Hq] targets: KV head hk of sequence b takes the next G rows of its sequence's list, distinct within the head, -1 where
    the list runs out (that head gets random input and is held to the bound only).  Returns (targets, done)."""
    t = torch.full((B, Hkv * G), -1, dtype=torch.int64)
    done = True
    for b in range(B):
        rows = rows_per_seq[b]
        for hk in range(Hkv):
            i0 = (it * Hkv + hk) * G
            for g in range(G):
                if i0 + g < len(rows):
                    t[b, hk * G + g] = rows[i0 + g]
            if (it * Hkv + hk + 1) * G < len(rows):
                done = False
    return t, done


def run_needles(ops, form, kv8, G, T, B, Hkv, seed):
    rows = form.startswith("rows") or form == "fused_rows"
    fused = form.startswith("fused")
    extra = form.endswith("extra")
    Hq = Hkv * G
    Tmax = 2 * T + 16 if rows else T + 8
    lens = [T, max(1, T // 3)] if rows else [T] * B
    B = len(lens) if rows else B
    len_for_split = Tmax if rows else T
    splits = ab.decode_splits(len_for_split, B, Hq, Hkv)
    per_seq = [nd.decode_targets(L, splits, extra=(L - 1,)) for L in lens]
    softcap, slopes = 0.0, None
    if extra:
        from oracle import decoder_oracle

        softcap = 30.0
        slopes = torch.from_numpy(decoder_oracle.alibi_slopes_reference(Hq) * min(1.0, 8.0 / T)).float()
    cos, sin = _rope(Tmax) if fused else (None, None)
    gen = torch.Generator().manual_seed(seed)
    it, worst, launches = 0, 0.0, 0
    while True:
        targets, done = deal_distinct(per_seq, B, Hkv, G, it)
        k = nd.pm1(gen, (B, Tmax, Hkv, D))
        v = torch.randn((B, Tmax, Hkv, D), generator=gen).half()
        pos = torch.tensor([L - 1 for L in lens], dtype=torch.int32)
        if fused:
            qkv = torch.empty((B, 1, (Hq + 2 * Hkv) * D), dtype=torch.float16)
            qkv[..., :Hq * D] = nd.pm1(gen, (B, 1, Hq * D)) * C
            qkv[..., Hq * D:(Hq + Hkv) * D] = nd.pm1(gen, (B, 1, Hkv * D))
            qkv[..., (Hq + Hkv) * D:] = torch.randn((B, 1, Hkv * D), generator=gen).half()
            for b in range(B):   # the new token's raw k = raw q / c of the head that targets it: both rotate at pos
                for hk in range(Hkv):
                    for g in range(G):
                        h = hk * G + g
                        if int(targets[b, h]) == int(pos[b]):
                            qkv[b, 0, (Hq + hk) * D:(Hq + hk + 1) * D] = qkv[b, 0, h * D:(h + 1) * D] / C
                            break
            qkv = qkv.cuda()
            z = torch.zeros((B, Tmax, Hkv, D), dtype=torch.float16, device="cuda")
            qrot = ops.rope_kv_append(qkv, z, z.clone(), cos, sin, 0, Hq, Hkv, D, D, pos_rows=pos.cuda())[:, 0].cpu()
            for b in range(B):
                for h in range(Hq):
                    t = int(targets[b, h])
                    if 0 <= t < int(pos[b]):
                        k[b, t, h // G] = qrot[b, h] / C
            q_ref = qrot
        else:
            q = nd.pm1(gen, (B, Hq, D)) * C
            for b in range(B):
                for h in range(Hq):
                    t = int(targets[b, h])
                    if t >= 0:
                        q[b, h] = k[b, t, h // G] * C
            q_ref = q
        kd, vd = k.cuda(), v.cuda()
        ks = vs = None
        if kv8:
            kd, ks = quant(k)
            vd, vs = quant(v)
        ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
        sl = slopes.cuda() if slopes is not None else None
        kw = dict(k_scale=ks, v_scale=vs)
        if fused:
            if rows:
                out = ops.decode_attention_rope(qkv, kd, vd, cos, sin, 0, Hq, Hkv, pos_rows=(ln - 1).contiguous(), max_len=Tmax, **kw)
            else:
                out = ops.decode_attention_rope(qkv, kd, vd, cos, sin, T - 1, Hq, Hkv, **kw)
        elif rows:
            out = ops.decode_attention(q.cuda(), kd, vd, 1, len_rows=ln, max_len=Tmax, softcap=softcap, alibi_slopes=sl, **kw)
        else:
            out = ops.decode_attention(q.cuda(), kd, vd, T, softcap=softcap, alibi_slopes=sl, **kw)
        kr = dequant(kd, ks) if kv8 else kd
        vr = dequant(vd, vs) if kv8 else vd
        want, bound = ab.decode_bound(q_ref.cuda(), kr, vr, lens, splits, softcap=softcap, alibi=sl)
        what = f"{form} kv8={kv8} G {G} T {T} splits {splits} launch {it}"
        ab.assert_attention_close(out, want, bound, what)
        worst = max(worst, ab.worst_ratio(out, want, bound))
        # the test must mean something: without its target row, each targeted head's reference moves > 100 bounds
        live = (targets >= 0) & (torch.tensor(lens).view(-1, 1) > 1)
        if bool(live.any()):
            drop = targets.clone().view(B, 1, Hq)
            pos_ref = torch.tensor(lens).view(-1, 1) - 1
            without = ab.reference(q_ref.cuda(), kr, vr, pos_ref, softcap=softcap, alibi=sl, drop=drop)["out"][:, 0]
            margin = ab.needle_margin(want, without, bound).cpu()
            assert bool((margin[live] > 100).all()), (what, float(margin[live].min()))
        launches += 1
        it += 1
        if done:
            return worst, launches


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_decode_needles(ops, form, kv8, G):
    worst = 0.0
    for T in LENGTHS:
        B, Hkv = (1, 16 // G) if form.startswith("rows") or form == "fused_rows" else (2, 16 // G)
        w, _ = run_needles(ops, form, kv8, G, T, B, Hkv, seed=T * 10 + G + 100 * FORMS.index(form) + 1000 * kv8)
        worst = max(worst, w)
    if G == 8 and form in ("plain", "fused"):   # the 64-split cap: B * Hkv = 1
        w, _ = run_needles(ops, form, kv8, G, 8192, 1, 1, seed=8192 + kv8)
        worst = max(worst, w)
    print(f"worst error / bound {form} kv8={kv8} G {G}: {worst:.3f}")


# ------------------------------------------------------------------ split counts through the C ABI

def _abi_call(L, ops, name, q, kc, vc, out, ks, vs, B, Hq, Hkv, T, Tmax, ws, nbytes, ln):
    p, st = ops._ptr, ops._stream()
    scale = D ** -0.5
    if name == "awq_decode_attention":
        return L.awq_decode_attention(p(q), p(kc), p(vc), p(out), None, T, T, B, Hq, Hkv, D, Tmax, scale, p(ws), nbytes, st)
    if name == "awq_decode_attention_ex":
        return L.awq_decode_attention_ex(p(q), p(kc), p(vc), p(out), None, T, T, B, Hq, Hkv, D, Tmax, scale, 30.0, None, p(ws),
                                         nbytes, st)
    if name == "awq_decode_attention_rows":
        return L.awq_decode_attention_rows(p(q), p(kc), p(vc), p(out), p(ln), Tmax, B, Hq, Hkv, D, Tmax, scale, 0.0, None, p(ws),
                                           nbytes, st)
    return L.awq_decode_attention_fp8(p(q), p(kc), p(vc), p(ks), p(vs), p(out), None, T, T, B, Hq, Hkv, D, Tmax, scale, p(ws),
                                      nbytes, st)


@pytest.mark.parametrize("name", ["awq_decode_attention", "awq_decode_attention_ex", "awq_decode_attention_rows",
                                  "awq_decode_attention_fp8"])
@pytest.mark.parametrize("B,Hkv,G,T", [(1, 2, 4, 1000), (4, 32, 1, 4096)])
def test_workspace_limited_split_counts(ops, name, B, Hkv, G, T):
    """workspace_bytes claimed for 1, 2, 3, 7 splits and the full count (the buffer is always the full size); (4, 32, 1, 4096):
    AWQ_ATTN_BLOCKS clamps the count to 8"""
    from autoawq_amd import _lib

    L = _lib.lib()
    Hq = Hkv * G
    Tmax = T if name != "awq_decode_attention_rows" else T + 200
    full = ab.decode_splits(Tmax if name.endswith("rows") else T, B, Hq, Hkv)
    per = B * Hq * (D + 2) * 4
    ws = torch.empty(L.awq_decode_attention_workspace_bytes(B, Hq), dtype=torch.uint8, device="cuda")
    rows = nd.decode_targets(T, full, extra=(T // 2,))
    targets, _ = nd.deal(rows, B, Hq)
    q, k, v = nd.decode_needles(B, Hkv, G, Tmax, targets, seed=B + T)
    kc, vc = k.cuda(), v.cuda()
    ks = vs = None
    if name.endswith("fp8"):
        kc, ks = quant(k)
        vc, vs = quant(v)
    kr = dequant(kc, ks) if ks is not None else kc
    vr = dequant(vc, vs) if vs is not None else vc
    ln = torch.full((B,), T, dtype=torch.int32, device="cuda")
    qd = q.cuda()
    softcap = 30.0 if name.endswith("_ex") else 0.0
    for n in sorted(set(x for x in (1, 2, 3, 7, full) if x <= full)):
        nbytes = per * n if n < full else ws.numel()
        assert nbytes <= ws.numel()
        splits = ab.decode_splits(Tmax if name.endswith("rows") else T, B, Hq, Hkv, workspace_bytes=nbytes)
        assert splits == n
        out = torch.full((B, Hq, D), float("nan"), dtype=torch.float16, device="cuda")
        _lib.check(_abi_call(L, ops, name, qd, kc, vc, out, ks, vs, B, Hq, Hkv, T, Tmax, ws, nbytes, ln), name)
        want, bound = ab.decode_bound(qd, kr, vr, [T] * B, splits, softcap=softcap)
        ab.assert_attention_close(out, want, bound, f"{name} {n} splits")
    if B * Hkv == 128:
        assert full == 8


# ------------------------------------------------------------------ dynamic range (plain form)

def _lin(T, rising):
    x = torch.linspace(-1.0, 1.0, T)
    return x if rising else x.flip(0)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("case", ["score90", "rising", "falling", "equal", "alibi_underflow", "softcap_saturated"])
def test_decode_dynamic_range(ops, case, kv8):
    B, Hkv, G, T = 1, 2, 4, 4096
    Hq = Hkv * G
    gen = torch.Generator().manual_seed(17)
    softcap, sl = 0.0, None
    v = torch.randn((B, T, Hkv, D), generator=gen).half()
    splits = ab.decode_splits(T, B, Hq, Hkv)
    if case in ("score90", "softcap_saturated"):
        targets, _ = nd.deal(nd.decode_targets(T, splits), B, Hq)
        q, k, v = nd.decode_needles(B, Hkv, G, T, targets, c=8.0, seed=17)
        softcap = 5.0 if case == "softcap_saturated" else 0.0
    elif case in ("rising", "falling"):   # the maximum moves on every row (rising) or sits in the prefetch set (falling)
        k = (_lin(T, case == "rising").view(1, T, 1, 1) * torch.ones((B, T, Hkv, D))).half()
        q = torch.full((B, Hq, D), 2.0, dtype=torch.float16)
    elif case == "equal":                 # every score 0: the output is mean(V)
        k = torch.zeros((B, T, Hkv, D), dtype=torch.float16)
        q = torch.randn((B, Hq, D), generator=gen).half()
    else:                                 # slope 1/2 over 4096 rows: the early rows' weights underflow
        k = torch.randn((B, T, Hkv, D), generator=gen).half()
        q = torch.randn((B, Hq, D), generator=gen).half()
        sl = torch.full((Hq,), 0.5)
    kc, vc = k.cuda(), v.cuda()
    ks = vs = None
    if kv8:
        kc, ks = quant(k)
        vc, vs = quant(v)
    kr = dequant(kc, ks) if kv8 else kc
    vr = dequant(vc, vs) if kv8 else vc
    out = ops.decode_attention(q.cuda(), kc, vc, T, softcap=softcap, alibi_slopes=sl.cuda() if sl is not None else None,
                               k_scale=ks, v_scale=vs)
    want, bound = ab.decode_bound(q.cuda(), kr, vr, [T], splits, softcap=softcap, alibi=sl.cuda() if sl is not None else None)
    ab.assert_attention_close(out, want, bound, case)
    if case == "equal":
        assert torch.allclose(want, vr[:, :T].double().mean(1).repeat_interleave(G, 1), atol=1e-12)


# ------------------------------------------------------------------ prefill

@pytest.mark.parametrize("start", [0, 63, 1000])
def test_prefill_needles(ops, start):
    """GQA 8:1, three sequences; targets on the diagonal, the KV-tile boundaries, the chunk start; anti-needles past the
    diagonal of rows = 3 mod 4 (31 / 63 / 127: wave and block boundaries).  Every output element against the fp64 reference."""
    B, S, Hq, Hkv = 3, 300, 8, 1
    Tmax = start + S + 8
    q, k, v, tgt = nd.prefill_needles(B, S, Hq, Hkv, start, Tmax, seed=start)
    k[:, start + S:] = float("nan")
    v[:, start + S:] = float("nan")
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    out = ops.prefill_attention(qd, kd, vd, start)
    want, bound = ab.prefill_bound(qd, kd, vd, start)
    ab.assert_attention_close(out, want, bound, f"prefill needles start {start}")
    without, _ = ab.prefill_bound(qd, kd, vd, start, drop=tgt)
    margin = ab.needle_margin(want, without, bound)[:, 1 if start == 0 else 0:]   # (query 0 of start 0 sees one row only)
    assert float(margin.min()) > 100, float(margin.min())
    print(f"worst error / bound prefill start {start}: {ab.worst_ratio(out, want, bound):.3f}")


@pytest.mark.parametrize("case", ["rising", "underflow"])
def test_prefill_dynamic_range(ops, case):
    B, S, Hq, Hkv, start = 2, 260, 8, 2, 100
    T = start + S
    gen = torch.Generator().manual_seed(5)
    v = torch.randn((B, T, Hkv, D), generator=gen).half()
    if case == "rising":   # the running maximum rises in every KV tile
        k = (_lin(T, True).view(1, T, 1, 1) * torch.ones((B, T, Hkv, D))).half()
        q = torch.full((B, S, Hq, D), 2.0, dtype=torch.float16)
    else:                  # scores +-90: most fp16 probabilities underflow
        k = nd.pm1(gen, (B, T, Hkv, D))
        q = nd.pm1(gen, (B, S, Hq, D)) * 8
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    out = ops.prefill_attention(qd, kd, vd, start)
    want, bound = ab.prefill_bound(qd, kd, vd, start)
    ab.assert_attention_close(out, want, bound, case)
