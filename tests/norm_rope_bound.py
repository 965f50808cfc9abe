"""float64 references, adversarial rows and derived windows for the two pieces of decode-step arithmetic next to the matmuls:
RMSNorm (four implementations) and RoPE + KV append (two), for the tests.

Notation: u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u); 1.01 covers the second-order products of the first-order
terms (all below 1e-4 here).  numpy converts float64 to float16 with ONE round-to-nearest-even, overflow to inf included, and that
conversion is monotone: a value known to lie in a real interval rounds into the interval of the rounded ends.  So both bounds are
WINDOWS of fp16 values, not distances: most of the time the two ends are the same fp16 number and the kernel has to hit it.

RMSNorm:  y = h w / sqrt(mean(h^2) + fp32(eps)),  h = x or fp16(x + r)
---------------------------------------------------------------------
`norm_reference` evaluates that in float64 with IEEE rules for inf and NaN (a row holding an inf has 1 / sqrt = 0: its finite
elements give 0, the inf itself NaN; a NaN poisons its row).  h = fp16(x + r) is one rounding of the exact sum (the kernels add in
fp32 and round to fp16: 24 >= 2 * 11 + 2 bits, so the double rounding is innocuous and both give the same bits).

Every implementation computes fp16(fp32(fp32(h) * inv) * fp32(w)), inv = rsqrtf(ss / H + eps), ss a fp32 sum of the H squares.
A square of an fp16 value has 22 significant bits and lies in [2^-48, 2^32]: exact in fp32, whether or not the compiler contracts
`ss += h * h` into an fma.  Only the additions round, all terms are positive, so a chain of n additions on the longest path from
a square to ss leaves ss within the RELATIVE error gamma(n); `/ H` and `+ eps` (eps > 0: the sum's relative error only shrinks)
add two.  inv = arg^(-1/2) carries HALF the relative error of its argument (first order; the 1.01 covers the rest).  rsqrtf is
1 ulp by the HIP math API, counted as 2 (4 u) as tests/matmul_bound.py counts it; the two multiplies round once each (2 u;
|h inv| <= sqrt(H) <= 128 and |w| <= 65504: no fp32 overflow, and the smallest product 2^-24 * 2^-24 * inv is fp32-normal).

    N_impl = ceil((n_sum + 2) / 2) + 4 + 2,        e = 1.01 gamma(N_impl)
    a correct kernel's output lies in [fp16(|y| (1 - e)), fp16(|y| (1 + e))] with the sign of y   (`norm_window`)

n_sum per implementation, from its code:
  * awq_rmsnorm_kernel (autoawq_amd/csrc/decoder.hip:135-174): thread t adds the 8 squares of each of its chunks t, t + 256, ...
    one after the other (:145-158): 8 ceil(H / 2048); wave_sum's butterfly 6 (:45-49, :159); red[0] + red[1] + red[2] + red[3]
    (:162) 3:                       n_sum = 8 ceil(H / 2048) + 9      (`depth_rmsnorm`: 14 at H <= 2048 .. 42 at H = 16384)
  * gemv_mfma's NORM staging with its own statistic pass (autoawq_amd/csrc/gemv_mfma.hip:276-293): the same per-thread chain
    over chunks tid, tid + NTHR, ... (:278-283), the butterfly 6 (:285), and `tot` over the block's waves starting from 0
    (:290-291): NWAVES.  The launch does not report NWAVES (4 or 8, gemv_config :792): the larger of the two totals,
                                    n_sum = max over NWAVES in (4, 8) of 8 ceil(K / (512 NWAVES)) + 6 + NWAVES   (`depth_mfma_norm`)
  * the same staging fed by the producer's ssq_out (`depth_mfma_ssq`): the producing block's thread holds ONE quad of its row's
    256-column tile (M <= 4: quads of row m are wave m, :488-489), ((o0^2 + o1^2) + o2^2) + o3^2 and the add to 0 (:486,
    :500-501, :552-553): 4; the wave's butterfly 6 (:493): a tile partial is within gamma(SSQ_TILE_N = 10) of the float64 sum
    of squares of the tile's STORED values.  The consumer's wave m sums <= 64 partials by a butterfly, 6 (:270-272), and `tot`
    adds it to 0 (:291): 1.      n_sum = 10 + 7 = 17
  * FX_NORM of gemv_rows (autoawq_amd/csrc/gemv_rows.hip:413-427, :463-473): derived in tests/matmul_bound.py, n_sum = 38, taken
    as N = 32 (matmul_bound.NORM_N, the default of matmul_bound.norm_prologue, which is built on `norm_window`).

RoPE:  lo = a c - b s,  hi = a s + b c  on the pair (i, i + rot / 2),  c, s the fp32 table entries of the row's position
--------------------------------------------------------------------------------------------------------------------------
rope_kv_append_body (decoder.hip:209-218) and the FUSED rotation of awq_decode_attn_kernel (:373-389) both convert the fp32 value of
awq_rope_term (awq_device.h: the product with the cosine rounded on its own, the product with the sine inside an fma) to fp16.  The
window does not lean on that choice: two products and a sum round once each, at most u |a c| + u |b s| + u |result| <=
2 u (|a c| + |b s|) to first order, with an fma one product less.  Taken as e_lo = 3 u (|a c| + |b s|), e_hi = 3 u (|a s| + |b c|):
every contraction of the expression fits (before awq_rope_term the two kernels had taken different ones), and the window is
[fp16(lo - e_lo), fp16(lo + e_lo)].  On rows that cancel (a c ~ b s) the window stays 3 u (|a c| + |b s|) wide while the result
is small: a kernel that rounds its products to fp16 first (2^-11 each) is far outside.  Dims >= rot and all of v are copies:
compared as bits, NaN payloads and signed zeros included.  A NaN in a rotated pair makes both members NaN, nothing else.
`cache_image` lays rows out in a whole cache around a sentinel, so a test compares EVERY element of the cache.

The tables are the kernel's input (RoPE.__init__, autoawq_amd/modules/fused/attn.py:48-55, the reference's fp32 outer(t, freqs)):
how they are built is not under test here.
"""
import numpy as np

U = 2.0 ** -24
SSQ_TILE_N = 10       # a producer's tile partial: 4 (one quad's squares and the add to 0) + 6 (butterfly)
NORM_KINDS = ("normal", "tiny", "subnormal", "outlier", "huge", "zero")   # + "nonfinite" for the stand-alone kernel
ROPE_KINDS = ("normal", "cancel", "big", "subnormal", "special")
F16_MAX = 65504.0


def gamma(n):
    return n * U / (1.0 - n * U)


def _f16(a):
    """float64 -> the float64 value of its fp16 rounding (one round-to-nearest-even; overflow gives inf)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------ RMSNorm

def norm_depth(n_sum):
    """N_impl of a statistic with n_sum additions on its longest path (docstring)"""
    return (n_sum + 2 + 1) // 2 + 4 + 2


def depth_rmsnorm(H):
    return norm_depth(8 * ((H + 2047) // 2048) + 9)


def depth_mfma_norm(K):
    return norm_depth(max(8 * ((K + 512 * nw - 1) // (512 * nw)) + 6 + nw for nw in (4, 8)))


def depth_mfma_ssq():
    return norm_depth(SSQ_TILE_N + 7)


def ssq_tiles_reference(y16):
    """[M, tiles] float64: the sums of squares of y16's 256-column tiles (the last one may be short)"""
    M, H = y16.shape
    tiles = (H + 255) // 256
    y = np.zeros((M, tiles * 256))
    y[:, :H] = np.asarray(y16, np.float16).astype(np.float64)
    return (y.reshape(M, tiles, 256) ** 2).sum(-1)


def stream_sum(x16, r16):
    """fp16(x + r): one rounding of the exact sum"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(x16, np.float16).astype(np.float64) + np.asarray(r16, np.float16).astype(np.float64)).astype(np.float16)


def norm_reference(x16, w16, eps, residual16=None):
    """y [M, H] float64 (docstring); with a residual (y, h), h [M, H] fp16 the stream that was normalised"""
    h = np.asarray(x16, np.float16) if residual16 is None else stream_sum(x16, residual16)
    h64 = h.astype(np.float64)
    with np.errstate(all="ignore"):
        y = h64 * np.asarray(w16, np.float16).astype(np.float64) / np.sqrt((h64 ** 2).mean(-1, keepdims=True) + float(np.float32(eps)))
    return y if residual16 is None else (y, h)


def norm_window(y, depth):
    """(lo, hi) float64 [M, H], fp16 values (or +-inf): the fp16 outputs a kernel of that depth may store; NaN where y is NaN"""
    e = 1.01 * gamma(depth)
    a = np.abs(y)
    near, far = _f16(a * (1.0 - e)), _f16(a * (1.0 + e))
    neg = np.signbit(y)
    return np.where(neg, -far, near), np.where(neg, -near, far)


def assert_in_window(got, lo, hi, what="", nan=None):
    """lo <= got <= hi element by element; NaN exactly where `nan` (default: where lo is NaN) says"""
    got = np.asarray(got).astype(np.float64)
    nan = np.isnan(lo) if nan is None else nan
    with np.errstate(invalid="ignore"):
        bad = np.where(nan, ~np.isnan(got), ~((got >= lo) & (got <= hi)))
    if bad.any():
        idx = np.argwhere(bad)[:8]
        where = ", ".join(f"{tuple(int(v) for v in i)}: {got[tuple(i)]!r} not in [{lo[tuple(i)]!r}, {hi[tuple(i)]!r}]" for i in idx)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} outside the window; first at {where}")


def outside(got, lo, hi, nan=None):
    """the mask assert_in_window raises on"""
    got = np.asarray(got).astype(np.float64)
    nan = np.isnan(lo) if nan is None else nan
    with np.errstate(invalid="ignore"):
        return np.where(nan, ~np.isnan(got), ~((got >= lo) & (got <= hi)))


def worst_ratio(got, want, lo, hi):
    """largest |got - want| / half-width over the finite elements, the half-width taken as the larger distance from the exact
    value to the window's ends (0 / 0 counts as 0: an exactly representable value that was hit)"""
    got = np.asarray(got).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.isfinite(got) & np.isfinite(want) & np.isfinite(lo) & np.isfinite(hi)
        err = np.abs(got - want)
        half = np.maximum(hi - want, want - lo)
        r = np.where(err == 0, 0.0, err / half)
    return float(r[ok].max()) if ok.any() else 0.0


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _subnormals(rng, shape):
    """fp16 subnormals of both signs, magnitude j 2^-24 with 1 <= j < 512 (so that the sum of two stays subnormal)"""
    return (rng.integers(1, 512, shape) * rng.choice([-1.0, 1.0], shape) * 2.0 ** -24).astype(np.float16)


def norm_rows(kind, M, H, seed=0):
    """h [M, H] fp16 of one kind (module docstring of the tests; `nonfinite` is made by norm_nonfinite)"""
    rng = _rng(seed, M, H, (NORM_KINDS + ("nonfinite",)).index(kind))
    normal = (2.0 * rng.standard_normal((M, H))).astype(np.float16)
    if kind == "normal":
        return normal
    if kind == "tiny":
        return (rng.standard_normal((M, H)) * 2.0 ** -9).astype(np.float16)
    if kind == "subnormal":
        return _subnormals(rng, (M, H))
    if kind == "outlier":
        h = rng.standard_normal((M, H)).astype(np.float16)
        h[np.arange(M), rng.integers(0, H, M)] = np.float16(F16_MAX)
        return h
    if kind == "huge":
        return (rng.uniform(50000.0, 65000.0, (M, H)) * rng.choice([-1.0, 1.0], (M, H))).astype(np.float16)
    assert kind == "zero"
    normal[0::2] = 0  # (M = 1: the zero row alone)
    return normal


def split_rows(h, seed=0):
    """(x, r) fp16 with fp16(x + r) of h's kind: r = fp16(t h), 1/4 <= t <= 3/4, x = fp16(h - r) (exact zeros stay zero, the
    sum of two subnormals is exact, |fp16(x + r) - h| <= 2^-9 |h|: two roundings)"""
    rng = _rng(seed, h.size)
    r = (h.astype(np.float64) * rng.uniform(0.25, 0.75, h.shape)).astype(np.float16)
    r[np.abs(h.astype(np.float64)) > 65000.0] = 0  # (the outlier 65504 stays itself: a sum of 65520 would round to inf)
    x = (h.astype(np.float64) - r.astype(np.float64)).astype(np.float16)
    return x, r


def norm_nonfinite(M, H, seed=0):
    """(x, r) fp16 [M, H]: row 0 (mod 3) holds one NaN, row 1 one +inf, row 2 a finite pair whose sum overflows fp16 (without the
    residual that row is an ordinary one)"""
    rng = _rng(seed, M, H, 99)
    x = rng.standard_normal((M, H)).astype(np.float16)
    r = rng.standard_normal((M, H)).astype(np.float16)
    for m in range(M):
        k = int(rng.integers(0, H))
        if m % 3 == 0:
            x[m, k] = np.float16(np.nan)
        elif m % 3 == 1:
            x[m, k] = np.float16(np.inf)
        else:
            x[m, k] = r[m, k] = np.float16(60000.0)
    return x, r


def norm_weights(H, seed=0, big=True):
    """[H] fp16: both signs, exact zeros, and (big) a few of magnitude 100 and 30000.  |h inv| <= sqrt(H) <= 128, so a weight
    of 100 never overflows fp16; 30000 does on every |h inv| > 2.18 and not below: the window then admits inf only where
    |y| (1 +- e) straddles 65520."""
    rng = _rng(seed, H, 7)
    w = ((rng.random(H) + 0.5) * rng.choice([-1.0, 1.0], H)).astype(np.float16)
    w[rng.random(H) < 1.0 / 16] = 0
    w[1 % H] = 0
    if big:
        n = max(1, H // 64)
        w[rng.integers(0, H, n)] = np.float16(100.0)
        w[rng.integers(0, H, n)] = np.float16(-100.0)
        w[rng.integers(0, H, n)] = np.float16(30000.0)
        w[H - 2] = np.float16(100.0)
        w[H - 3] = np.float16(-30000.0)
    return w


# ------------------------------------------------------------------ RoPE

def rope_tables(rot, max_pos, theta):
    """(cos, sin) fp32 [max_pos, rot / 2] numpy, built as RoPE.__init__ builds them (attn.py:48-55) -- the kernel's input"""
    import torch

    if rot == 0:
        z = np.zeros((max_pos, 0), np.float32)
        return z, z.copy()
    freqs = 1.0 / (theta ** (torch.arange(0, rot, 2)[: (rot // 2)].float() / rot))
    f = torch.outer(torch.arange(max_pos), freqs).float()
    return f.cos().contiguous().numpy(), f.sin().contiguous().numpy()


def rope_reference(src16, cos32, sin32, pos, rot):
    """src16 [..., D] fp16 head rows, pos an integer array that broadcasts against src16.shape[:-1] -> (lo, hi, e_lo, e_hi)
    float64 [..., rot / 2]: the exact rotation of the pairs (i, i + rot / 2) and the window half-widths (docstring)"""
    src = np.asarray(src16, np.float16).astype(np.float64)
    hr = rot // 2
    pos = np.broadcast_to(np.asarray(pos, np.int64), src.shape[:-1])
    c, s = np.asarray(cos32, np.float32).astype(np.float64)[pos], np.asarray(sin32, np.float32).astype(np.float64)[pos]
    a, b = src[..., :hr], src[..., hr:rot]
    with np.errstate(invalid="ignore"):
        return a * c - b * s, a * s + b * c, 3 * U * (np.abs(a * c) + np.abs(b * s)), 3 * U * (np.abs(a * s) + np.abs(b * c))


def rope_window(src16, cos32, sin32, pos, rot, rotate=True):
    """(lo, hi, exact) [..., D]: lo / hi fp16 arrays -- the ends of the window in the rotated dims (NaN where the result is NaN), the
    source itself elsewhere -- and exact bool: compare as bits (the pass-through dims, or every dim with rotate=False: a v row)"""
    src16 = np.ascontiguousarray(src16, np.float16)
    lo, hi, exact = src16.copy(), src16.copy(), np.ones(src16.shape, bool)
    if rotate and rot:
        l, h, el, eh = rope_reference(src16, cos32, sin32, pos, rot)
        hr = rot // 2
        with np.errstate(over="ignore", invalid="ignore"):
            lo[..., :hr], hi[..., :hr] = (l - el).astype(np.float16), (l + el).astype(np.float16)
            lo[..., hr:rot], hi[..., hr:rot] = (h - eh).astype(np.float16), (h + eh).astype(np.float16)
        exact[..., :rot] = False
    return lo, hi, exact


def cache_image(sentinel, rows, pos, counts=None):
    """The expected cache: `sentinel` [B', Tmax, Hkv, D] everywhere except rows (b, pos[b] + s, h) = rows[b, s, h] for the slots
    s < counts[b] (default: all S) -- rows [B, S, Hkv, D], pos [B]"""
    img = np.array(sentinel, copy=True)
    B, S = rows.shape[:2]
    for b in range(B):
        n = S if counts is None else int(counts[b])
        for s in range(n):
            img[b, int(pos[b]) + s] = rows[b, s]
    return img


def assert_rows_in_window(got16, lo16, hi16, exact, what=""):
    """got16 fp16 against a window image: bits where `exact`, else lo <= got <= hi with NaN exactly where the window is NaN"""
    got16 = np.asarray(got16, np.float16)
    bad = got16.view(np.uint16) != lo16.view(np.uint16)  # (most elements are the sentinel's or the window's lower end: bits first)
    idx = np.nonzero(bad & ~exact)
    bad[idx] = outside(got16[idx], lo16[idx].astype(np.float64), hi16[idx].astype(np.float64))
    if bad.any():
        idx = np.argwhere(bad)[:8]
        where = ", ".join(f"{tuple(int(v) for v in i)}: {got16[tuple(i)]!r} ({'bits of ' if exact[tuple(i)] else 'window '}"
                          f"{lo16[tuple(i)]!r} .. {hi16[tuple(i)]!r})" for i in idx)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} elements wrong; first at {where}")


def rope_ratio(got16, src16, cos32, sin32, pos, rot):
    """worst |got - exact| / e over the rotated dims with a finite, non-zero e"""
    if not rot:
        return 0.0
    l, h, el, eh = rope_reference(src16, cos32, sin32, pos, rot)
    got = np.asarray(got16).astype(np.float64)
    want, e = np.concatenate([l, h], -1), np.concatenate([el, eh], -1)
    # the window's ends are fp16 roundings of want -+ e: the half-width is e plus the rounding of the end
    with np.errstate(invalid="ignore", over="ignore"):
        half = np.maximum(_f16(want + e) - want, want - _f16(want - e))
        ok = np.isfinite(got[..., :rot]) & np.isfinite(half) & (half > 0)
        r = np.abs(got[..., :rot] - want) / half
    return float(r[ok].max()) if ok.any() else 0.0


SPECIALS = np.array([0x7E00, 0x7E01, 0xFE55, 0x7D00, 0x7C01, 0x7C00, 0xFC00, 0x8000], np.uint16).view(np.float16)
# quiet and signalling NaNs with distinct payloads, +inf, -inf, -0


def rope_rows(kind, B, S, Hq, Hkv, D, rot, cos32, sin32, pos, seed=0):
    """qkv [B, S, (Hq + 2 Hkv) D] fp16 of one kind; pos [B]: token (b, s) sits at pos[b] + s (`cancel` needs the angle).  Every
    kind carries SPECIALS in its pass-through dims and in the v rows of every other token."""
    assert kind in ROPE_KINDS
    rng = _rng(seed, B, S, Hq, Hkv, D, rot, ROPE_KINDS.index(kind))
    H = Hq + 2 * Hkv
    hr = rot // 2
    x = rng.standard_normal((B, S, H, D)).astype(np.float16)
    P = (np.asarray(pos, np.int64)[:, None] + np.arange(S)[None, :])[:, :, None]  # [B, S, 1]
    rk = x[:, :, :Hq + Hkv]  # the q and k heads (a view)
    if kind == "cancel" and rot:
        a = (50.0 * rng.standard_normal((B, S, Hq + Hkv, hr))).astype(np.float16)
        c = np.broadcast_to(cos32[P].astype(np.float64), a.shape)
        s = np.broadcast_to(sin32[P].astype(np.float64), a.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = a.astype(np.float64) * c / s
        ok = (np.abs(s) > 1e-3) & (np.abs(b) < 60000.0)
        rk[..., :hr] = a
        rk[..., hr:rot] = np.where(ok, b, rk[..., hr:rot].astype(np.float64)).astype(np.float16)
    elif kind == "big":
        x[:] = (rng.uniform(30000.0, F16_MAX, x.shape) * rng.choice([-1.0, 1.0], x.shape)).astype(np.float16)
    elif kind == "subnormal":
        x[:] = _subnormals(rng, x.shape)
    elif kind == "special" and rot:
        rk[..., 0::3, 0] = np.float16(0.0)        # +-0 on either side of a pair
        rk[..., 1::3, hr] = np.float16(-0.0)
        if hr > 1:
            rk[..., 0::2, 1] = np.float16(np.nan)  # a NaN in the first member of pair 1 ...
            rk[..., 1::2, hr + hr - 1] = np.float16(np.nan)  # ... and in the second member of the last pair
        else:
            rk[..., 0::2, 0] = np.float16(np.nan)
    n = len(SPECIALS)
    for d in range(rot, D):  # pass-through dims of q and k
        rk[..., d] = np.where((np.arange(Hq + Hkv) + d) % 3 == 0, SPECIALS[d % n], rk[..., d])
    v = x[:, :, Hq + Hkv:]
    tok = (np.arange(B)[:, None] * S + np.arange(S)[None, :]) % 2 == 0
    for j in range(min(n, D)):
        d = (j * 5 + 1) % D
        v[..., d] = np.where(tok[:, :, None], SPECIALS[j], v[..., d])
    return np.ascontiguousarray(x.reshape(B, S, H * D))


# ------------------------------------------------------------------ the cases the GPU tests run (the CPU tests prove the bound on the same)

EPSS = (1e-5, 1e-6)
RMSNORM_H = (8, 136, 2048, 2056, 4096, 16376, 16384)   # 16-byte chunks: 1, 17, 256 (one per thread), 257, 512, 2047, 2048 = MAXC * 256
RMSNORM_M = (1, 3)
# awq_gemm_forward_normed takes K % 32 == 0 with K % g == 0 (awq_gemv_mfma_supports, gemv_mfma.hip:742-750; gemm_layout, capi.hip:21):
# 32 and 64 are the smallest two, at g = 32 -- 4 and 8 chunks, far below a block.  2176 = 272 chunks: more than a 256-thread
# block, not a multiple of 256 or 512; 4096 = 512 chunks: a multiple of both block sizes.
MFMA_NORM_SHAPES = ((32, 256, 32), (64, 256, 32), (2176, 256, 128), (4096, 256, 128))   # (K, N, g)
MFMA_NORM_M = (1, 2, 4)
MFMA_NORM_KINDS = ("normal", "tiny", "subnormal", "outlier")
SSQ_SHAPES = ((256, 512, 128), (256, 288, 32), (128, 4096, 128))   # (I, H, g): 2 tiles; 2 tiles, the last of 32 columns; 16 tiles
SSQ_M = (1, 3, 4)
SSQ_KINDS = ("normal", "tiny")
ROWS_NORM_SHAPES = ((4096, 40, 128), (12288, 8, 128))   # FX_SHAPE of test_gpu_matmul_bounds; the largest K FX_NORM takes (gemv_rows.hip:721)
ROWS_NORM_KINDS = ("tiny", "subnormal")

ROPE_DIMS = ((128, 128), (128, 64), (128, 0), (64, 64), (96, 32), (80, 80), (256, 256), (256, 254), (2, 2))
ROPE_HEADS = ((8, 2), (3, 3), (1, 1))
ROPE_BS = ((1, 1), (3, 3))
ROPE_THETAS = (1e4, 5e5, 1e6)
FUSED_POSITIONS = (0, 57, 2047)
FUSED_KINDS = ("normal", "cancel", "big", "subnormal")
FUSED_TMAX = 2056


def rope_tmax(D):
    return 4096 if D == 128 else 64


def rope_positions(D, S):
    T = rope_tmax(D)
    return (0, 1, 57, 2047, T - S) if D == 128 else (0, 1, 57, T - S)


def row_positions(pos, B, S, Tmax):
    """a different position per sequence, every row inside the cache"""
    step = 5 if pos + 5 * (B - 1) + S <= Tmax else -5
    return [pos + step * b for b in range(B)]


def rope_cases(D, rot):
    """The (Hq, Hkv, B, S, theta, Tmax, pos, kind, counts) of one (D, rot): every position and kind, with the head counts, batch
    shapes and thetas dealt round so that each value and most pairs of values occur.  counts [B]: the *_rows_n form's new tokens
    per sequence (0 and S among them)."""
    i = ROPE_DIMS.index((D, rot))
    for (B, S) in ROPE_BS:
        for pos in rope_positions(D, S):
            for kind in ROPE_KINDS:
                Hq, Hkv = ROPE_HEADS[i % 3]
                theta = ROPE_THETAS[(i // 3) % 3]
                counts = [S, 0, max(S - 2, 0)][:B] if B > 1 else [S if i % 2 == 0 else 0]
                yield Hq, Hkv, B, S, theta, rope_tmax(D), pos, kind, counts
                i += 1


def record(impl, shape, kind, eps, ratio):
    """NORM_ROPE_BOUND_RECORD=<file>: one line per GPU case -- implementation, shape, kind, eps, worst error / window half-width
    (matmul forms: error / bound).  Recorded, never asserted."""
    import os

    line = f"{impl} {shape} {kind} eps={eps:g} {ratio:.4f}"
    print(line)
    path = os.environ.get("NORM_ROPE_BOUND_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
