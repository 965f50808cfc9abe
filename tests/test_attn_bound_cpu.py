"""The attention bound of tests/attn_bound.py is neither too loose nor too tight (CPU only).

  * the fp64 reference agrees with oracle/decoder_oracle.py;
  * positive control: fp32 emulations of the kernels' order of operations -- decode: rows dealt to the splits with the kernel's
    chunk formula and the host's split count, an online softmax per lane group, lane-group / wave merges, the combine; prefill:
    64-row KV tiles, fp16 P relative to the running maximum, the denominator from the rounded P -- pass the bound;
  * mutations of those emulations (a dropped row at the prefetch set, the split boundaries and T - 1, a stale empty split given
    full weight, splits merged without the maximum, a causal diagonal shifted for one wave, the soft cap after ALiBi, an ALiBi
    bias of the wrong sign) fail it on the needle inputs of tests/attn_needles.py, and the dropped row fails it on random inputs
    at T = 4096 as well.
"""
import numpy as np
import pytest
import torch

import attn_bound as ab
import attn_needles as nd

SCALE = 128 ** -0.5


# ------------------------------------------------------------------ fp32 emulations

def _merge(m1, l1, o1, m2, l2, o2):
    mn = torch.maximum(m1, m2)
    ca = torch.where(m1 == -np.inf, torch.zeros_like(m1), torch.exp(m1 - mn))
    cb = torch.where(m2 == -np.inf, torch.zeros_like(m2), torch.exp(m2 - mn))
    return mn, l1 * ca + l2 * cb, o1 * ca[..., None] + o2 * cb[..., None]


def emulate_decode(q, k, v, lens, splits, softcap=0.0, alibi=None, mut=None):
    """awq_decode_attn_kernel + awq_decode_attn_combine_kernel in fp32.  q [B, Hq, D] fp16, k / v [B, Tmax, Hkv, D] (fp16 or the
    exact fp8 values as fp32), lens [B].  mut: None or (name, arg):
      ("drop", (b, hk, t))   row t of KV head hk of sequence b is skipped
      ("stale_empty", v_prev) an empty split is not written: it keeps the partial split 0 of an earlier call (on the V cache
                             v_prev) left in the reused workspace, and the combine weights it as live
      ("no_max", None)       the combine weights a split by exp(m_s) instead of exp(m_s - max)
      ("cap_after_alibi", None), ("alibi_sign", None), ("alibi_shift", +-1): the score modifiers mis-ordered / mis-signed / the
                             bias measured from pos -+ 1"""
    name, arg = mut if mut else (None, None)
    B, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    qf = q.float() * np.float32(SCALE)
    out = torch.empty((B, Hq, D), dtype=torch.float16)
    hmap = torch.arange(Hq) // G
    for b in range(B):
        T = int(lens[b])
        kb = k[b, :T].float()[:, hmap]                                     # [T, Hq, D]
        vb = v[b, :T].float()[:, hmap]
        s = torch.einsum("hd,thd->ht", qf[b], kb)                          # fp32 [Hq, T]
        t = torch.arange(T, dtype=torch.float32)
        pos = T - 1
        if alibi is not None:
            sl = torch.as_tensor(alibi, dtype=torch.float32).view(Hq, 1)
            shift = arg if name == "alibi_shift" else 0
            bias = sl * (t - (pos + shift)).view(1, T)
            if name == "alibi_sign":
                bias = -bias
        if softcap and name == "cap_after_alibi":
            s = softcap * torch.tanh((s + bias) * np.float32(1.0 / softcap))
        else:
            if softcap:
                s = softcap * torch.tanh(s * np.float32(1.0 / softcap))
            if alibi is not None:
                s = s + bias
        chunk = ab.decode_chunk(T, splits)
        steps = (chunk + 15) // 16
        t0 = torch.arange(splits) * chunk
        t1 = torch.clamp(t0 + chunk, max=T)

        def partials(vb):
            m = torch.full((Hq, splits, 16), -np.inf)
            lsum = torch.zeros((Hq, splits, 16))
            o = torch.zeros((Hq, splits, 16, D))
            lane = torch.arange(16)
            for j in range(steps):
                tt = t0.view(-1, 1) + lane.view(1, -1) + 16 * j                   # [splits, 16]
                live = (tt < t1.view(-1, 1)).expand(Hq, splits, 16).clone()
                if name == "drop":
                    db, dh, dt = arg
                    if db == b:
                        live[dh * G:(dh + 1) * G] &= (tt != dt).view(1, splits, 16)
                tc = tt.clamp(max=T - 1)
                sc = s[:, tc]                                                  # [Hq, splits, 16]
                vv = vb[tc].permute(2, 0, 1, 3)                                # [Hq, splits, 16, D]
                mn = torch.maximum(m, sc)
                corr, p = torch.exp(m - mn), torch.exp(sc - mn)
                lsum = torch.where(live, lsum * corr + p, lsum)
                o = torch.where(live[..., None], o * corr[..., None] + p[..., None] * vv, o)
                m = torch.where(live, mn, m)
            # lane groups o = 4 w + r: merge r with r ^ 1, then r ^ 2 (the xor-16 / xor-32 shuffles), then the four waves
            m, lsum, o = m.view(Hq, splits, 4, 4), lsum.view(Hq, splits, 4, 4), o.view(Hq, splits, 4, 4, D)
            for x in (1, 2):
                idx = torch.arange(4) ^ x
                m, lsum, o = _merge(m, lsum, o, m[..., idx], lsum[..., idx], o[..., idx, :])
            m, lsum, o = m[..., 0], lsum[..., 0], o[..., 0, :]                  # [Hq, splits, 4(waves)]
            mw = m.amax(-1)
            acc, ls = torch.zeros((Hq, splits, D)), torch.zeros((Hq, splits))
            for w in range(4):
                cw = torch.where(m[..., w] == -np.inf, torch.zeros_like(mw), torch.exp(m[..., w] - mw))
                acc = acc + o[..., w, :] * cw[..., None]
                ls = ls + lsum[..., w] * cw
            return mw, ls, acc

        mw, ls, acc = partials(vb)
        if splits == 1:
            out[b] = (acc[:, 0] / ls[:, :1]).half()
            continue
        if name == "stale_empty":
            pm, pl, pa = partials(arg[b, :T].float()[:, hmap])   # split 0 of the previous call on cache `arg`
            empty = (t0 >= T).view(1, -1)
            mw = torch.where(empty, pm[:, :1], mw)
            ls = torch.where(empty, pl[:, :1], ls)
            acc = torch.where(empty[..., None], pa[:, :1], acc)
        mx = mw.amax(-1, keepdim=True)
        if name == "no_max":
            wgt = torch.where(mw == -np.inf, torch.zeros_like(mw), torch.exp(mw))
        else:
            wgt = torch.where(mw == -np.inf, torch.zeros_like(mw), torch.exp(mw - mx))
        den = (ls * wgt).sum(-1, keepdim=True)
        num = torch.zeros((Hq, D))
        for sp in range(splits):
            num = num + acc[:, sp] * wgt[:, sp:sp + 1]
        out[b] = (num / den).half()
    return out


def emulate_prefill(q, k, v, start, diag_shift_rows=None):
    """awq_prefill_attn_kernel in fp32: 64-row KV tiles, running maximum in log2 units, P = fp16(exp2(s * sc2 - m)) relative to
    it, numerator and denominator (the ones-MFMA) from the same rounded P.  diag_shift_rows (r0, r1): query rows r0 .. r1 - 1 also
    see KV row start + s + 1 (the causal mask off by one for those rows only)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    hmap = torch.arange(Hq) // G
    kv_len = start + S
    sc2 = np.float32(SCALE * 1.44269504088896)
    qf = q.float().permute(0, 2, 1, 3)                                     # [B, Hq, S, D]
    kf = k[:B, :kv_len].float()[:, :, hmap].permute(0, 2, 1, 3)             # [B, Hq, T, D]
    vf = v[:B, :kv_len].float()[:, :, hmap].permute(0, 2, 1, 3)
    qpos = start + torch.arange(S).view(S, 1)
    lim = qpos.clone()
    if diag_shift_rows is not None:
        lim[diag_shift_rows[0]:diag_shift_rows[1]] += 1
    m = torch.full((B, Hq, S, 1), -np.inf)
    lacc = torch.zeros((B, Hq, S, 1))
    oacc = torch.zeros((B, Hq, S, D))
    for kv0 in range(0, kv_len, 64):
        kt = kf[:, :, kv0:kv0 + 64]
        s = qf @ kt.transpose(-1, -2)                                       # fp32 [B, Hq, S, n]
        tt = kv0 + torch.arange(kt.shape[2]).view(1, -1)
        s = s.masked_fill(tt > lim, -np.inf)
        mloc = s.amax(-1, keepdim=True)
        m_new = torch.maximum(m, mloc * sc2)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s * sc2 - m_new).half().float()
        m = m_new
        oacc = oacc * alpha + p @ vf[:, :, kv0:kv0 + 64]
        lacc = lacc * alpha + p.sum(-1, keepdim=True)
    return (oacc / lacc).half().permute(0, 2, 1, 3)


def _dec_ref(q, k, v, lens, splits, **kw):
    return ab.decode_bound(q, k.float(), v.float(), lens, splits, **kw)


def _fails(got, want, bound):
    return bool((~((got.double() - want).abs() <= bound)).any())


# ------------------------------------------------------------------ the reference

def test_reference_matches_oracle():
    from oracle import decoder_oracle

    gen = torch.Generator().manual_seed(11)
    B, Hq, Hkv, T = 2, 8, 2, 45
    q = torch.randn((B, Hq, 128), generator=gen).half()
    kc = torch.randn((B, T + 3, Hkv, 128), generator=gen).half()
    vc = torch.randn((B, T + 3, Hkv, 128), generator=gen).half()
    slopes = decoder_oracle.alibi_slopes_reference(Hq)
    for softcap, alibi in ((0.0, None), (20.0, slopes)):
        want = decoder_oracle.attention_reference(q.numpy(), kc.numpy(), vc.numpy(), T, softcap=softcap, alibi_slopes=alibi)
        got = ab.reference(q, kc, vc, torch.full((B, 1), T - 1), softcap=softcap,
                           alibi=None if alibi is None else torch.from_numpy(alibi))["out"][:, 0]
        assert np.abs(got.numpy() - want).max() <= 1e-12
    S, start = 7, 20
    qp = torch.randn((B, S, Hq, 128), generator=gen).half()
    want = decoder_oracle.prefill_attention_reference(qp.numpy(), kc.numpy(), vc.numpy(), start, list(range(S)))
    got, _ = ab.prefill_bound(qp, kc, vc, start)
    assert np.abs(got.numpy() - want).max() <= 1e-12


# ------------------------------------------------------------------ positive controls

@pytest.mark.parametrize("B,Hkv,G,T,max_len", [(1, 2, 4, 1, 1), (2, 2, 4, 65, 65), (1, 2, 8, 257, 257), (1, 4, 2, 1000, 1000),
                                               (1, 2, 4, 4096, 4096), (2, 1, 1, 100, 2048), (1, 1, 4, 8192, 8192)])
def test_decode_emulation_passes_on_random_inputs(B, Hkv, G, T, max_len):
    gen = torch.Generator().manual_seed(T + G)
    Hq = Hkv * G
    q = torch.randn((B, Hq, 128), generator=gen).half()
    k = torch.randn((B, T, Hkv, 128), generator=gen).half()
    v = torch.randn((B, T, Hkv, 128), generator=gen).half()
    splits = ab.decode_splits(max_len, B, Hq, Hkv)
    lens = [T] * B
    want, bound = _dec_ref(q, k, v, lens, splits)
    ab.assert_attention_close(emulate_decode(q, k, v, lens, splits), want, bound, f"T {T} splits {splits}")


@pytest.mark.parametrize("softcap,alibi", [(30.0, False), (0.0, True), (8.0, True)])
def test_decode_emulation_passes_with_modifiers(softcap, alibi):
    from oracle import decoder_oracle

    gen = torch.Generator().manual_seed(3)
    B, Hkv, G, T = 2, 2, 4, 700
    q = (torch.randn((B, Hkv * G, 128), generator=gen) * 2).half()
    k = torch.randn((B, T, Hkv, 128), generator=gen).half()
    v = torch.randn((B, T, Hkv, 128), generator=gen).half()
    sl = torch.from_numpy(decoder_oracle.alibi_slopes_reference(Hkv * G)).float() if alibi else None
    splits = ab.decode_splits(T, B, Hkv * G, Hkv)
    want, bound = _dec_ref(q, k, v, [T, T], splits, softcap=softcap, alibi=sl)
    got = emulate_decode(q, k, v, [T, T], splits, softcap=softcap, alibi=sl)
    ab.assert_attention_close(got, want, bound, "modifiers")


@pytest.mark.parametrize("splits", [1, 2, 3, 7, 32])
def test_decode_emulation_passes_on_needles(splits):
    B, Hkv, G, T = 1, 4, 8, 4096
    targets, _ = nd.deal(nd.decode_targets(T, splits), B, Hkv * G)
    q, k, v = nd.decode_needles(B, Hkv, G, T, targets, seed=splits)
    want, bound = _dec_ref(q, k, v, [T], splits)
    ab.assert_attention_close(emulate_decode(q, k, v, [T], splits), want, bound, f"needles, {splits} splits")


@pytest.mark.parametrize("B,S,Hq,Hkv,start", [(1, 300, 8, 1, 0), (2, 129, 4, 2, 63), (1, 200, 4, 4, 1000)])
def test_prefill_emulation_passes(B, S, Hq, Hkv, start):
    gen = torch.Generator().manual_seed(S + start)
    q = torch.randn((B, S, Hq, 128), generator=gen).half()
    k = torch.randn((B, start + S, Hkv, 128), generator=gen).half()
    v = torch.randn((B, start + S, Hkv, 128), generator=gen).half()
    want, bound = ab.prefill_bound(q, k, v, start)
    ab.assert_attention_close(emulate_prefill(q, k, v, start), want, bound, "random")
    q, k, v, _ = nd.prefill_needles(B, S, Hq, Hkv, start, start + S, seed=start)
    want, bound = ab.prefill_bound(q, k, v, start)
    ab.assert_attention_close(emulate_prefill(q, k, v, start), want, bound, "needles")


# ------------------------------------------------------------------ needle generators

def test_needles_carry_the_weight():
    B, Hkv, G, T = 2, 2, 4, 4096
    for softcap in (0.0, 30.0):
        targets, _ = nd.deal(nd.decode_targets(T, 32), B, Hkv * G)
        q, k, v = nd.decode_needles(B, Hkv, G, T, targets, seed=1)
        q2, k2, v2 = nd.decode_needles(B, Hkv, G, T, targets, seed=1)
        assert torch.equal(q, q2) and torch.equal(k, k2) and torch.equal(v, v2)   # deterministic
        w = ab.target_weight(q, k, v, torch.full((B, 1), T - 1), targets.view(B, 1, -1), softcap=softcap)
        assert float(w.min()) >= 0.5, (softcap, float(w.min()))
    for start in (0, 63, 1000):
        q, k, v, tgt = nd.prefill_needles(3, 300, 8, 1, start, start + 300, seed=start)
        w = ab.target_weight(q, k, v, (start + torch.arange(300)).view(1, -1).expand(3, -1), tgt)
        assert float(w.min()) >= 0.5, start


# ------------------------------------------------------------------ mutations

def _old_tol_ok(got, want):
    return float((got.double() - want).abs().max()) <= 2e-3 * float(want.abs().max()) + 2 ** -11


@pytest.mark.parametrize("splits", [1, 3, 32])
def test_dropped_row_fails_on_needles(splits):
    B, Hkv, G, T = 1, 4, 8, 4096
    rows = nd.decode_targets(T, splits)
    targets, _ = nd.deal(rows, B, Hkv * G)
    q, k, v = nd.decode_needles(B, Hkv, G, T, targets, seed=splits)
    want, bound = _dec_ref(q, k, v, [T], splits)
    for h in range(Hkv * G):
        t, hk = int(targets[0, h]), h // G
        got = emulate_decode(q, k, v, [T], splits, mut=("drop", (0, hk, t)))
        assert _fails(got, want, bound), (splits, t)


def test_dropped_row_fails_on_random_inputs_at_4096():
    """no needle: one KV head's row lost in a random N(0, 1) cache, at every position the needle tests target"""
    B, Hkv, G, T = 1, 2, 4, 4096
    gen = torch.Generator().manual_seed(4096)
    q = torch.randn((B, Hkv * G, 128), generator=gen).half()
    k = torch.randn((B, T, Hkv, 128), generator=gen).half()
    v = torch.randn((B, T, Hkv, 128), generator=gen).half()
    splits = ab.decode_splits(T, B, Hkv * G, Hkv)
    want, bound = _dec_ref(q, k, v, [T], splits)
    ab.assert_attention_close(emulate_decode(q, k, v, [T], splits), want, bound, "unmutated")
    for t in (0, 127, 128, 2047, 2048, T - 1):
        assert _fails(emulate_decode(q, k, v, [T], splits, mut=("drop", (0, 1, t))), want, bound), t


def test_stale_empty_split_fails():
    """max_len 2048 (16 splits) over a 100-row sequence: splits 2 .. 15 are empty (chunk 16 -> rows 0 .. 99 in splits 0 .. 6)"""
    B, Hkv, G, T = 1, 2, 4, 100
    splits = ab.decode_splits(2048, B, Hkv * G, Hkv)
    assert ab.decode_chunk(T, splits) * 7 >= T and splits > 7
    targets, _ = nd.deal([0, 5, 15, 16, 31, 50, 98, 99], B, Hkv * G)
    q, k, v = nd.decode_needles(B, Hkv, G, T, targets, seed=7)
    want, bound = _dec_ref(q, k, v, [T], splits)
    ab.assert_attention_close(emulate_decode(q, k, v, [T], splits), want, bound, "unmutated")
    assert _fails(emulate_decode(q, k, v, [T], splits, mut=("stale_empty", -v)), want, bound)


def test_merge_without_the_max_fails():
    """scores ~90 (c = 8): exp(m_s) overflows fp32 where exp(m_s - max) does not"""
    B, Hkv, G, T = 1, 2, 4, 1000
    splits = ab.decode_splits(T, B, Hkv * G, Hkv)
    targets, _ = nd.deal(nd.decode_targets(T, splits), B, Hkv * G)
    q, k, v = nd.decode_needles(B, Hkv, G, T, targets, c=8.0, seed=8)
    want, bound = _dec_ref(q, k, v, [T], splits)
    ab.assert_attention_close(emulate_decode(q, k, v, [T], splits), want, bound, "unmutated")
    assert _fails(emulate_decode(q, k, v, [T], splits, mut=("no_max", None)), want, bound)


def test_prefill_diagonal_shift_of_one_wave_fails():
    """query rows 32 .. 63 (wave 1 of the first block) also see row start + s + 1: the anti-needles of rows 35, 39, .., 63"""
    for start in (0, 63):
        B, S, Hq, Hkv = 1, 160, 8, 1
        q, k, v, _ = nd.prefill_needles(B, S, Hq, Hkv, start, start + S, seed=start)
        want, bound = ab.prefill_bound(q, k, v, start)
        ab.assert_attention_close(emulate_prefill(q, k, v, start), want, bound, "unmutated")
        got = emulate_prefill(q, k, v, start, diag_shift_rows=(32, 64))
        bad = ~((got.double() - want).abs() <= bound)
        rows = sorted(set(int(r) for r in torch.nonzero(bad.any(-1).any(-1).any(0)).flatten()))
        assert rows == list(range(35, 64, 4)), rows


def _extra_needles(T=1000, Hkv=2, G=4):
    from oracle import decoder_oracle

    splits = ab.decode_splits(T, 1, Hkv * G, Hkv)
    targets, _ = nd.deal(nd.decode_targets(T, splits), 1, Hkv * G)
    q, k, v = nd.decode_needles(1, Hkv, G, T, targets, seed=9)
    sl = torch.from_numpy(decoder_oracle.alibi_slopes_reference(Hkv * G)).float()
    return q, k, v, splits, sl


def test_softcap_after_alibi_fails():
    q, k, v, splits, sl = _extra_needles()
    want, bound = _dec_ref(q, k, v, [1000], splits, softcap=30.0, alibi=sl)
    ab.assert_attention_close(emulate_decode(q, k, v, [1000], splits, softcap=30.0, alibi=sl), want, bound, "unmutated")
    assert _fails(emulate_decode(q, k, v, [1000], splits, softcap=30.0, alibi=sl, mut=("cap_after_alibi", None)), want, bound)


def test_alibi_sign_fails_and_a_shifted_origin_is_no_bug():
    """slope * (pos - t) fails.  slope * (t - pos -+ 1) adds the same constant to every score of the head: the softmax cannot see
    it (an off-by-one in ALiBi's origin is not a bug of the output), and the bound accepts it -- the bias of the test inputs is
    large (slopes up to 1/2, 1000 rows), so the shifted fp32 scores still differ in rounding."""
    q, k, v, splits, sl = _extra_needles()
    want, bound = _dec_ref(q, k, v, [1000], splits, softcap=30.0, alibi=sl)
    assert _fails(emulate_decode(q, k, v, [1000], splits, softcap=30.0, alibi=sl, mut=("alibi_sign", None)), want, bound)
    for d in (1, -1):
        ab.assert_attention_close(emulate_decode(q, k, v, [1000], splits, softcap=30.0, alibi=sl, mut=("alibi_shift", d)),
                                  want, bound, f"shift {d}")


def test_old_tolerance_misses_what_the_bound_catches():
    """The dropped row on random inputs at T = 4096: the new bound catches it at each of 16 positions, the old decode tolerance
    (2e-3 max|want| + 2^-11) lets several of them through (6 of these 16)."""
    B, Hkv, G, T = 1, 2, 4, 4096
    gen = torch.Generator().manual_seed(4096)
    q = torch.randn((B, Hkv * G, 128), generator=gen).half()
    k = torch.randn((B, T, Hkv, 128), generator=gen).half()
    v = torch.randn((B, T, Hkv, 128), generator=gen).half()
    splits = ab.decode_splits(T, B, Hkv * G, Hkv)
    want, bound = _dec_ref(q, k, v, [T], splits)
    missed = 0
    for t in range(0, T, 256):
        got = emulate_decode(q, k, v, [T], splits, mut=("drop", (0, 1, t)))
        assert _fails(got, want, bound), t
        missed += _old_tol_ok(got, want)
    assert missed >= 4, missed
