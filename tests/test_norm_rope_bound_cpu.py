"""tests/norm_rope_bound.py proves itself on the CPU: float32 restatements of the four RMSNorm orders and of RoPE under the three
fma contractions stay inside their windows on every kind, shape and eps the GPU tests run; named defects leave the window, on the
kinds each test names; the two eps values are told apart on the quiet rows; and the new references agree with the ones the
suite already pins (tests/golden/rope_golden.npz, oracle.decoder_oracle.rmsnorm_reference)."""
import numpy as np
import pytest

import norm_rope_bound as nrb
from conftest import golden

F32 = np.float32


# ------------------------------------------------------------------ float32 restatements of the kernels' order of operations

def butterfly(v):
    """__shfl_xor sums over the last axis (a power of two), offsets n/2 .. 1; every lane ends with the same bits"""
    n = v.shape[-1]
    o = n // 2
    while o:
        v = v + v[..., np.arange(n) ^ o]
        o //= 2
    return v[..., 0]


def rsqrt32(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(a.astype(np.float64))).astype(F32)


def thread_sums(h32, nthr):
    """[M, nthr]: thread t adds the 8 squares of its chunks t, t + nthr, ... one after the other"""
    M, H = h32.shape
    per = -(-(H // 8) // nthr)
    x = np.zeros((M, per * nthr * 8), F32)
    x[:, :H] = h32
    x = x.reshape(M, per, nthr, 8)
    ss = np.zeros((M, nthr), F32)
    for i in range(per):
        for e in range(8):
            ss = ss + x[:, i, :, e] * x[:, i, :, e]
    return ss


def finish(h32, w32, tot, H, eps, defect=None):
    eps = F32(eps)
    with np.errstate(all="ignore"):
        if defect == "eps_over_h":
            inv = rsqrt32(tot / F32(H) + eps / F32(H))
        elif defect == "eps_outside":
            inv = (F32(1.0) / (np.sqrt(tot / F32(H)) + eps)).astype(F32)
        elif defect == "h_minus_8":
            inv = rsqrt32(tot / F32(H - 8) + eps)
        else:
            inv = rsqrt32(tot / F32(H) + eps)
        if defect == "xw_fp16":
            return ((h32 * w32[None]).astype(np.float16).astype(F32) * inv[:, None]).astype(np.float16)
        return (h32 * inv[:, None] * w32[None]).astype(np.float16)


def emu_rmsnorm(h16, w16, eps, defect=None):
    """awq_rmsnorm_kernel (decoder.hip:135-174)"""
    h32, w32 = h16.astype(F32), w16.astype(F32)
    with np.errstate(all="ignore"):
        red = butterfly(thread_sums(h32, 256).reshape(-1, 4, 64))
        tot = red[:, 0] + red[:, 1] + red[:, 2]
        if defect != "wave_dropped":
            tot = tot + red[:, 3]
    return finish(h32, w32, tot, h16.shape[1], eps, defect)


def emu_mfma_norm(h16, w16, eps, nwaves):
    """gemv_mfma's NORM staging with its own statistic pass (gemv_mfma.hip:276-304)"""
    h32, w32 = h16.astype(F32), w16.astype(F32)
    with np.errstate(all="ignore"):
        part = butterfly(thread_sums(h32, 64 * nwaves).reshape(-1, nwaves, 64))
        tot = np.zeros(h16.shape[0], F32)
        for w in range(nwaves):
            tot = tot + part[:, w]
    return finish(h32, w32, tot, h16.shape[1], eps)


def emu_ssq_tiles(y16):
    """the producer's ssq_out: [M, tiles] fp32 (gemv_mfma.hip:486-494)"""
    M, H = y16.shape
    tiles = (H + 255) // 256
    y = np.zeros((M, tiles * 256), F32)
    y[:, :H] = y16.astype(F32)
    q = y.reshape(M, tiles, 64, 4)
    with np.errstate(all="ignore"):
        ss = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
        return butterfly(np.zeros_like(ss) + ss)


def emu_mfma_ssq(h16, w16, eps, defect=None):
    """the NORM staging fed by ssq_in (gemv_mfma.hip:268-274, :289-304)"""
    ssq = emu_ssq_tiles(h16)
    if defect == "tile_dropped":
        ssq = ssq[:, :-1]
    lanes = np.zeros((h16.shape[0], 64), F32)
    lanes[:, :ssq.shape[1]] = ssq
    with np.errstate(all="ignore"):
        tot = np.zeros(h16.shape[0], F32) + butterfly(lanes)
    return finish(h16.astype(F32), w16.astype(F32), tot, h16.shape[1], eps)


def emu_rows_norm(h16, w16, eps):
    """FX_NORM of gemv_rows (gemv_rows.hip:413-427, :463-473): a lane's SL slots x 4 pieces x 4 v_dot2 (two roundings each: the pair
    sum, then the accumulate), the pieces added to `ss`; DPP sums inside the 16-lane rows, then (r0 + r1) + (r2 + r3).  Which
    chunk goes to which lane is the launch's business (cidx); here chunk (4 s + j) 64 + lane -- the depth is the same for any."""
    M, H = h16.shape
    SL = -(-H // 2048)
    x = np.zeros((M, SL * 2048), F32)
    x[:, :H] = h16.astype(F32)
    x = x.reshape(M, SL, 4, 64, 4, 2)
    with np.errstate(all="ignore"):
        ss = np.zeros((M, 64), F32)
        for s in range(SL):
            for j in range(4):
                q = np.zeros((M, 64), F32)
                for i in range(4):
                    q = (x[:, s, j, :, i, 0] * x[:, s, j, :, i, 0] + x[:, s, j, :, i, 1] * x[:, s, j, :, i, 1]) + q
                ss = ss + q
        r = butterfly(ss.reshape(M, 4, 16))
        tot = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    return finish(h16.astype(F32), w16.astype(F32), tot, H, eps)


def emu_rope(src16, cos32, sin32, pos, rot, mode="plain"):
    """rope_kv_append_body's rotation of head rows [..., D] (decoder.hip:209-218) in float32.  mode: `plain` (no fma), `fma_first` /
    `fma_second` (the first / second product of each expression stays exact inside an fma), or a defect."""
    out = np.array(src16, np.float16, copy=True)
    if not rot:
        return out
    hr, D = rot // 2, src16.shape[-1]
    pos = np.broadcast_to(np.asarray(pos, np.int64), src16.shape[:-1])
    if mode == "pos_off_by_one":
        pos = np.minimum(pos + 1, cos32.shape[0] - 1)
    if mode == "table_stride":  # row stride D / 2 instead of rot / 2 (the same table when rot == D)
        i = (pos[..., None] * (D // 2) + np.arange(hr)) % cos32.size
        c, s = cos32.reshape(-1)[i], sin32.reshape(-1)[i]
    else:
        c, s = cos32[pos], sin32[pos]
    if mode == "sin_sign":
        s = -s
    if mode == "interleaved":
        a, b = src16[..., 0:rot:2], src16[..., 1:rot:2]
    else:
        a, b = src16[..., :hr], src16[..., hr:rot]
    a32, b32, a64, b64, c64, s64 = a.astype(F32), b.astype(F32), a.astype(np.float64), b.astype(np.float64), c.astype(np.float64), s.astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == "fma_first":     # (fp16 x fp32 has 35 significant bits: exact in float64)
            lo, hi = (a64 * c64 - (b32 * s).astype(np.float64)).astype(F32), (a64 * s64 + (b32 * c).astype(np.float64)).astype(F32)
        elif mode == "fma_second":
            lo, hi = ((a32 * c).astype(np.float64) - b64 * s64).astype(F32), ((a32 * s).astype(np.float64) + b64 * c64).astype(F32)
        elif mode == "fp16_products":
            h = lambda v: v.astype(np.float16).astype(F32)
            lo, hi = h(a32 * c) - h(b32 * s), h(a32 * s) + h(b32 * c)
        else:
            lo, hi = a32 * c - b32 * s, a32 * s + b32 * c
        if mode == "interleaved":
            out[..., 0:rot:2], out[..., 1:rot:2] = lo.astype(np.float16), hi.astype(np.float16)
        else:
            out[..., :hr], out[..., hr:rot] = lo.astype(np.float16), hi.astype(np.float16)
    return out


# ------------------------------------------------------------------ RMSNorm: soundness

def norm_case(kind, M, H, seed=3):
    return nrb.norm_rows(kind, M, H, seed), nrb.norm_weights(H, seed)


@pytest.mark.parametrize("H", nrb.RMSNORM_H)
def test_rmsnorm_restatement_stays_inside_the_window(H):
    for M in nrb.RMSNORM_M:
        for kind in nrb.NORM_KINDS:
            h, w = norm_case(kind, M, H)
            for eps in nrb.EPSS:
                lo, hi = nrb.norm_window(nrb.norm_reference(h, w, eps), nrb.depth_rmsnorm(H))
                nrb.assert_in_window(emu_rmsnorm(h, w, eps), lo, hi, f"{kind} M{M} H{H} eps{eps}")
        # the residual form normalises fp16(x + r); the non-finite rows follow IEEE
        x, r = nrb.norm_nonfinite(M, H)
        for res in (None, r):
            y = nrb.norm_reference(x, w, 1e-5, res)
            y, hh = y if res is not None else (y, x)
            lo, hi = nrb.norm_window(y, nrb.depth_rmsnorm(H))
            nrb.assert_in_window(emu_rmsnorm(hh, w, 1e-5), lo, hi, f"nonfinite M{M} H{H}")
            assert np.isnan(y[0]).all()                                 # the NaN's row
            if M > 1:
                assert np.isnan(y[1]).sum() == 1 and (y[1][~np.isnan(y[1])] == 0).all()   # the inf's row: 0, NaN at the inf
                assert np.isfinite(y[2]).all() == (res is None)         # the overflowing sum: only with the residual


def test_split_rows_keeps_the_kind():
    for kind in nrb.NORM_KINDS:
        h = nrb.norm_rows(kind, 3, 2056, 3)
        x, r = nrb.split_rows(h)
        s = nrb.stream_sum(x, r).astype(np.float64)
        assert np.isfinite(s).all() and (np.abs(s - h.astype(np.float64)) <= 2.0 ** -9 * np.abs(h.astype(np.float64)) + 2.0 ** -24).all(), kind
        if kind == "subnormal":
            assert np.array_equal(s, h.astype(np.float64))
        if kind == "zero":
            assert not s[0::2].any() and s[1].any()
    assert (np.abs(nrb.norm_rows("subnormal", 3, 136, 3).astype(np.float64)) < 2.0 ** -14).all()


@pytest.mark.parametrize("K,N,g", nrb.MFMA_NORM_SHAPES)
def test_mfma_norm_restatement_stays_inside_the_window(K, N, g):
    for kind in nrb.MFMA_NORM_KINDS:
        h, w = nrb.norm_rows(kind, max(nrb.MFMA_NORM_M), K, 3), nrb.norm_weights(K, 3, big=False)
        for eps in nrb.EPSS:
            lo, hi = nrb.norm_window(nrb.norm_reference(h, w, eps), nrb.depth_mfma_norm(K))
            for nw in (4, 8):
                nrb.assert_in_window(emu_mfma_norm(h, w, eps, nw), lo, hi, f"{kind} K{K} eps{eps} waves{nw}")


@pytest.mark.parametrize("H", [s[1] for s in nrb.SSQ_SHAPES] + [16384])
def test_ssq_hand_over_restatement_stays_inside_its_bounds(H):
    for kind in nrb.SSQ_KINDS + ("subnormal", "outlier"):
        h, w = nrb.norm_rows(kind, max(nrb.SSQ_M), H, 3), nrb.norm_weights(H, 3, big=False)
        ssq = emu_ssq_tiles(h).astype(np.float64)
        want = nrb.ssq_tiles_reference(h)
        assert (np.abs(ssq - want) <= nrb.gamma(nrb.SSQ_TILE_N) * want).all(), kind
        for eps in nrb.EPSS:
            lo, hi = nrb.norm_window(nrb.norm_reference(h, w, eps), nrb.depth_mfma_ssq())
            nrb.assert_in_window(emu_mfma_ssq(h, w, eps), lo, hi, f"{kind} H{H} eps{eps}")


@pytest.mark.parametrize("K,N,g", nrb.ROWS_NORM_SHAPES)
def test_rows_norm_restatement_stays_inside_the_window(K, N, g):
    import matmul_bound as mb

    for kind in nrb.ROWS_NORM_KINDS + ("normal", "outlier"):
        h, w = nrb.norm_rows(kind, 1, K, 3), nrb.norm_weights(K, 3, big=False)
        for eps in nrb.EPSS:
            lo, hi = nrb.norm_window(nrb.norm_reference(h, w, eps), mb.NORM_N)
            nrb.assert_in_window(emu_rows_norm(h, w, eps), lo, hi, f"{kind} K{K} eps{eps}")


def test_norm_prologue_is_the_window():
    """matmul_bound.norm_prologue at a depth: x16 the fp16 of the exact value, slack the larger distance to the window's ends"""
    import matmul_bound as mb

    h, w = nrb.norm_rows("tiny", 2, 136, 3), nrb.norm_weights(136, 3, big=False)
    for depth in (mb.NORM_N, 16, 96):
        x16, slack = mb.norm_prologue(h, w, 1e-6, depth) if depth != mb.NORM_N else mb.norm_prologue(h, w, 1e-6)
        y = nrb.norm_reference(h, w, 1e-6)
        lo, hi = nrb.norm_window(y, depth)
        assert np.array_equal(x16, y.astype(np.float16))
        assert np.array_equal(slack, np.maximum(hi - x16.astype(np.float64), x16.astype(np.float64) - lo))
        assert (slack >= 0).all() and (slack == 0).mean() > 0.9  # (the window is one fp16 value nearly everywhere)


# ------------------------------------------------------------------ RMSNorm: the bound bites

# defect -> the kinds on which it must leave the window (M = 3, H = 2056, both eps; `tile_dropped`: H = 16384, 64 tiles, and 288)
NORM_DEFECTS = {
    "eps_over_h": ("normal", "tiny", "subnormal"),   # (`normal`: mean(h^2) = 4, the window is one fp16 value wide; not `outlier` / `huge`)
    "eps_outside": ("normal", "tiny", "subnormal"),
    "h_minus_8": ("normal", "tiny", "outlier", "huge"),       # 4 / H = 2e-3 on inv -- except where eps dominates (`subnormal`)
    "wave_dropped": ("normal", "tiny", "subnormal", "outlier", "huge"),
    "xw_fp16": ("normal", "tiny", "subnormal", "outlier", "huge"),
    "tile_dropped": ("normal", "tiny", "subnormal", "outlier", "huge"),
}


@pytest.mark.parametrize("defect", list(NORM_DEFECTS))
def test_norm_defect_leaves_the_window(defect):
    shapes = [(3, 16384), (3, 288)] if defect == "tile_dropped" else [(3, 2056)]
    caught = set()
    for M, H in shapes:
        for kind in nrb.NORM_KINDS:
            h, w = norm_case(kind, M, H)
            for eps in nrb.EPSS:
                y = nrb.norm_reference(h, w, eps)
                if defect == "tile_dropped":
                    got, depth = emu_mfma_ssq(h, w, eps, defect), nrb.depth_mfma_ssq()
                else:
                    got, depth = emu_rmsnorm(h, w, eps, defect), nrb.depth_rmsnorm(H)
                if nrb.outside(got, *nrb.norm_window(y, depth)).any():
                    caught.add(kind)
    print(defect, "caught on", sorted(caught))
    assert set(NORM_DEFECTS[defect]) <= caught, (defect, sorted(caught))


@pytest.mark.parametrize("impl", ["rmsnorm", "mfma_norm", "mfma_ssq", "rows_norm"])
def test_eps_needle(impl):
    """On the quiet kinds the two eps values give references further apart than the window is wide, on at least half of the
    elements with a non-zero weight: a kernel that ignores, scales or misplaces eps cannot pass both."""
    if impl == "rmsnorm":
        cases = [(M, H, nrb.depth_rmsnorm(H), True) for H in nrb.RMSNORM_H for M in nrb.RMSNORM_M]
    elif impl == "mfma_norm":
        cases = [(max(nrb.MFMA_NORM_M), K, nrb.depth_mfma_norm(K), False) for K, _, _ in nrb.MFMA_NORM_SHAPES]
    elif impl == "mfma_ssq":
        cases = [(max(nrb.SSQ_M), H, nrb.depth_mfma_ssq(), False) for _, H, _ in nrb.SSQ_SHAPES]
    else:
        import matmul_bound as mb

        cases = [(1, K, mb.NORM_N, False) for K, _, _ in nrb.ROWS_NORM_SHAPES]
    for M, H, depth, big in cases:
        for kind in ("tiny", "subnormal"):
            h, w = nrb.norm_rows(kind, M, H, 3), nrb.norm_weights(H, 3, big=big)
            ys = [nrb.norm_reference(h, w, eps) for eps in nrb.EPSS]
            with np.errstate(invalid="ignore"):  # (inf - inf where a weight of 30000 overflows: not live)
                width = np.maximum(*[np.subtract(*nrb.norm_window(y, depth)[::-1]) for y in ys])
            live = np.broadcast_to(w != 0, h.shape) & np.isfinite(width)
            apart = (np.abs(ys[0] - ys[1]) > width) & live
            assert apart.sum() >= 0.5 * live.sum(), (impl, kind, M, H, int(apart.sum()), int(live.sum()))


def test_norm_reference_rounds_to_the_oracle():
    from oracle import decoder_oracle

    for H in (8, 136, 2056):
        for kind in ("normal", "tiny", "subnormal", "outlier", "huge", "zero"):
            h, w = nrb.norm_rows(kind, 3, H, 3), nrb.norm_weights(H, 3, big=False)
            for eps in nrb.EPSS:
                lo, hi = nrb.norm_window(nrb.norm_reference(h, w, eps), nrb.depth_rmsnorm(H))
                nrb.assert_in_window(decoder_oracle.rmsnorm_reference(h, w, eps), lo, hi, f"{kind} H{H} eps{eps}")


# ------------------------------------------------------------------ RoPE

_tables = {}


def tables(rot, Tmax, theta):
    key = (rot, Tmax, theta)
    if key not in _tables:
        _tables[key] = nrb.rope_tables(rot, Tmax, theta)
    return _tables[key]


def rope_case(D, rot, case):
    """(qkv rows [B, S, H, D], positions [B, S, 1], tables) of one rope_cases entry, per-row positions"""
    Hq, Hkv, B, S, theta, Tmax, pos, kind, _ = case
    cos, sin = tables(rot, Tmax, theta)
    prow = nrb.row_positions(pos, B, S, Tmax)
    x = nrb.rope_rows(kind, B, S, Hq, Hkv, D, rot, cos, sin, prow, seed=5).reshape(B, S, Hq + 2 * Hkv, D)
    P = (np.asarray(prow)[:, None] + np.arange(S)[None, :])[:, :, None]
    return x[:, :, :Hq + Hkv], P, cos, sin


@pytest.mark.parametrize("D,rot", nrb.ROPE_DIMS)
def test_rope_restatements_stay_inside_the_window(D, rot):
    kinds = set()
    for case in nrb.rope_cases(D, rot):
        rk, P, cos, sin = rope_case(D, rot, case)
        lo, hi, exact = nrb.rope_window(rk, cos, sin, P, rot)
        for mode in ("plain", "fma_first", "fma_second"):
            nrb.assert_rows_in_window(emu_rope(rk, cos, sin, P, rot, mode), lo, hi, exact, f"{mode} {case}")
        kinds.add(case[7])
        if case[7] == "special" and rot:  # a NaN makes both members of its pair NaN and nothing else
            nan = np.isnan(rk[..., :rot].astype(np.float64))
            pair = nan[..., :rot // 2] | nan[..., rot // 2:]
            assert pair.any() and np.array_equal(np.isnan(lo[..., :rot].astype(np.float64)), np.concatenate([pair, pair], -1))
    assert kinds == set(nrb.ROPE_KINDS)


def test_cancel_rows_cancel_and_big_rows_overflow():
    case = (8, 2, 3, 3, 1e4, 4096, 57, "cancel", None)
    rk, P, cos, sin = rope_case(128, 128, case)
    lo, _, el, _ = nrb.rope_reference(rk, cos, sin, P, 128)
    assert np.median(np.abs(lo) / (el / (3 * nrb.U))) < 1e-3   # |a c - b s| << |a c| + |b s| on most pairs
    rk, P, cos, sin = rope_case(128, 128, case[:7] + ("big", None))
    wlo, whi, _ = nrb.rope_window(rk, cos, sin, P, 128)
    inf = np.isinf(wlo.astype(np.float64)) & np.isinf(whi.astype(np.float64))
    assert 0.01 < inf.mean() < 0.9


# defect -> kinds on which it must leave the window, at (D, rot) = (128, 64) -- partial rotation, so that the table stride differs
ROPE_DEFECTS = {
    "fp16_products": ("normal", "cancel", "big"),
    "sin_sign": ("normal", "cancel", "big", "subnormal", "special"),
    "interleaved": ("normal", "cancel", "big", "subnormal", "special"),
    "pos_off_by_one": ("normal", "cancel", "big", "subnormal", "special"),
    "table_stride": ("normal", "cancel", "big", "subnormal", "special"),
}


@pytest.mark.parametrize("defect", list(ROPE_DEFECTS))
def test_rope_defect_leaves_the_window(defect):
    caught, frac = set(), {}
    for case in nrb.rope_cases(128, 64):
        if case[6] == 0 and defect in ("sin_sign", "table_stride"):
            continue  # (position 0: sin = 0 and row 0 of the table whatever the stride)
        rk, P, cos, sin = rope_case(128, 64, case)
        lo, hi, exact = nrb.rope_window(rk, cos, sin, P, 64)
        got = emu_rope(rk, cos, sin, P, 64, defect)
        bad = got.view(np.uint16) != lo.view(np.uint16)
        bad &= np.where(exact, True, nrb.outside(got, lo.astype(np.float64), hi.astype(np.float64)))
        if bad.any():
            caught.add(case[7])
        frac.setdefault(case[7], []).append(float(bad[..., :64].mean()))
    print(defect, {k: round(max(v), 3) for k, v in frac.items()})
    assert set(ROPE_DEFECTS[defect]) <= caught, (defect, sorted(caught))
    if defect == "fp16_products":  # the reason for the `cancel` kind: most of a cancelling row fails, the smaller part of a Gaussian one
        assert max(frac["cancel"]) > 0.5 > max(frac["normal"])


@pytest.mark.parametrize("name", ["full", "partial", "late"])
def test_rope_window_contains_the_reference_class(name):
    """the q and k slices the reference project's own RoPE class produced lie in the windows of rope_reference"""
    g = golden("rope_golden")
    D, rot, start, S = [int(v) for v in g[f"{name}_meta"]]
    cos, sin = tables(rot, 64, 10000.0)
    P = (start + np.arange(S))[None, :, None]
    for src, out in ((g[f"{name}_xq"], g[f"{name}_q"]), (g[f"{name}_xk"], g[f"{name}_k"])):
        lo, hi, exact = nrb.rope_window(src, cos, sin, P, rot)
        nrb.assert_rows_in_window(out, lo[..., :rot], hi[..., :rot], exact[..., :rot], name)
        assert not exact[..., :rot].any() and exact[..., rot:].all()


def test_cache_image_places_rows_and_keeps_the_sentinel():
    rng = np.random.default_rng(0)
    sent = rng.standard_normal((3, 16, 2, 4)).astype(np.float16)
    rows = rng.standard_normal((2, 3, 2, 4)).astype(np.float16)
    img = nrb.cache_image(sent, rows, [5, 13], counts=[3, 0])
    assert np.array_equal(img[0, 5:8], rows[0]) and np.array_equal(img[1], sent[1]) and np.array_equal(img[2], sent[2])
    assert np.array_equal(img[0, :5], sent[0, :5]) and np.array_equal(img[0, 8:], sent[0, 8:])
    img = nrb.cache_image(sent, rows, [0, 13])
    assert np.array_equal(img[1, 13:16], rows[1]) and np.array_equal(img[0, :3], rows[0]) and np.array_equal(sent[0, :3] != img[0, :3], np.ones((3, 2, 4), bool))
