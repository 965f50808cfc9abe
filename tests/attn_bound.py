"""fp64 attention reference and a per-element error bound derived from the attention kernels' arithmetic, for the tests.

`reference` computes softmax(scale q k^T [soft cap] [+ ALiBi]) v in torch float64 on whatever device its inputs live on, for any
number of query rows per sequence: query row (b, r) sees the cache rows t <= pos[b, r].  Decode is R = 1 with pos = length - 1
(FUSED forms: the new token's position); prefill is R = S with pos = start + s.  `decode_bound` / `prefill_bound` return it with
the bound beside it, `assert_attention_close` compares a kernel's output with both.

Notation: u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u), s_t the exact score of row t (soft cap and ALiBi applied),
M = max_t s_t, p_t = exp(s_t - M), out = sum p_t v_t / sum p_t.

The bound (both kernel classes)
-------------------------------
Both kernels compute out~ = sum p~_t v_t / sum p~_t with the SAME perturbed weights p~_t in numerator and denominator (decode: the
one fp32 p feeds l and the accumulator; prefill: the ones-MFMA sums the same fp16 P the numerator uses).  A weight perturbation
p~_t = p_t + e_t therefore moves the output by sum e_t (v_t - out) / sum p_t (first order; a factor common to every p~_t cancels,
which is why the maximum a partial is taken against never matters, only each row's own error).  With |e_t| <= w_t:

    |out~ - out| <= ulp16(out) + 1.01 * [ sum w_t (|v_t| + |out|) / sum p           (weights: per-row errors; |v_t - out| <= |v_t| + |out|)
                                          + 2 gamma(N) sum p_t |v_t| / sum p        (fp32 accumulation of numerator and denominator)
                                          + 4 u |out| ]                             (the final division and its reciprocal)

ulp16(x) = max(|x|, 2^-14) 2^-10 covers the one fp16 rounding of the output (half an ulp of the fp32 value, which sits within the
other terms of the exact one).  1.01 covers the second-order products of the first-order terms (all of them < 1e-2 here).

Per-row weight error w_t = p_t eps_t (+ a_t, prefill):
  * score error delta_t: the q k dot product in fp32 from exact fp16 (or exactly dequantised fp8) products, depth n_dot:
        gamma(n_dot) * scale * sum_e |q_e k_te|
    plus, when a soft cap or ALiBi is on, one rounding each of s / cap, tanh (<= 4 u, OCML tanh is within 2 ulp), cap * tanh,
    slope * (t - pos) and the sum -- the cap's derivative is <= 1, so input errors pass through unamplified:
        8 u (|s_raw| + |s_capped| + |bias| + |s_t|)   (generous: 8 u per term where the count is 2 .. 5 roundings).
    A score error delta moves p_t by the factor e^delta: relative error delta_t.
  * exp error: every exp the kernel evaluates (the row's own p and each rescale factor its partial later meets, at most n_exp of
    them) is v_exp_f32 (<= 1 ulp; taken as 2 ulps = 4 u) of an argument x rounded once or twice (relative error u |x| each,
    i.e. 2 u |x| in the result).  The arguments of one row's chain telescope: they sum to M~ - s_t, so
        eps_exp,t <= 4 u n_exp + 4 u (M - s_t)      (4 u instead of 2 u per unit of M - s_t: the fp32 M~ and s~ differ from M, s)
  * eps_t = delta_t + eps_exp,t.  Rows whose fp32 p underflows (s_t - M < -87) are off by < 2^-126 relative to the maximum row,
    far below every term above; a_t = 0 for decode.

Decode class: awq_decode_attn_kernel + awq_decode_attn_combine_kernel (csrc/decoder.hip), fp16 and fp8 caches
------------------------------------------------------------------------------------------------------------------------
  * q f = fp32(q * scale) (one rounding), 8 fmas in the lane, the 16-lane butterfly (4 adds); an fp8 cache multiplies the sum by
    the row's scale, a power of two (exact).  n_dot = 1 + 8 + 4 + 1 = 14.
  * A lane group walks the rows t0 + o + 16 j of its split (o in 0..15) one at a time: o := o * corr + p v (two roundings), and l
    likewise; the four lane groups of a wave merge in 2 levels (2 roundings each), the four waves in a running sum (4), the
    splits in the combine kernel's running sum (nsplit); an fp8 cache's p * scale_v is exact (power of two), counted once anyway:
        N = 2 ceil(chunk / 16) + 4 + 4 + nsplit + 2,      chunk = the kernel's own split size (decoder.hip, `chunk <= 0`).
  * n_exp = ceil(chunk / 16) (the running corrections of a lane) + 2 (lane merges) + 1 (waves) + 1 (combine) + 1 (the row's p).
  * fp8: the dequantised values code * 2^k are exact in fp32, so the bound is the same on the dequantised cache
    (tests/kv8_ref.py::dequantize).  FUSED forms: the rotated q passes through fp16; the reference takes q from the fp16 append.

Prefill class: awq_prefill_attn_kernel (csrc/prefill_attn.hip)
--------------------------------------------------------------
  * S^T = K Q^T: four v_mfma_f32_16x16x32_f16 steps of 32 exact fp16 products into fp32; the MFMA's internal order is not
    specified, so each step counts as 33 sequential roundings: n_dot = 4 * 33 = 132 (the scale enters through one fma).
  * P = fp16(exp2(s log2e - m_run)), m_run the running maximum of the query row at that tile.  fp16 rounding: <= 2^-11 P for
    P >= 2^-14, <= 2^-25 absolute below (subnormals and the flush to 0).  Later tiles multiply P by alpha = exp2(m_run - m_new)
    <= 1, and m_run never exceeds the final maximum, so in units of the final maximum the error is <= 2^-11 p_t + 2^-25:
        w_t = p_t (eps_t + 2^-11) + 2^-25 over the visible rows.
    The denominator is built from the same rounded P (ones-MFMA), so this is a weight perturbation like the others.
  * O and l: per 64-row tile two MFMA steps (33 roundings each, same reason) and one rescale by alpha: N = 67 ntiles.
  * n_exp = ntiles (one alpha per tile) + 1.
"""
import numpy as np
import torch

U = 2.0 ** -24

DECODE_N_DOT = 14
PREFILL_N_DOT = 132


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp16(x):
    return torch.clamp(x.abs(), min=2.0 ** -14) * 2.0 ** -10


# ------------------------------------------------------------------ the decode launch (decoder.hip: awq_launch_decode_attention)

def decode_splits(len_for_split, B, Hq, Hkv, workspace_bytes=None, blocks=1024, rows=128, single=256):
    """Split count of the launch: AWQ_ATTN_SINGLE / _ROWS / _BLOCKS, the 64-split cap, and the workspace-limited count the C ABI
    gives a smaller workspace (workspace_bytes None = large enough)."""
    splits = 1 if len_for_split <= single else (len_for_split + rows - 1) // rows
    splits = min(splits, max(blocks // (B * Hkv), 1))
    splits = min(max(splits, 1), 64)
    per = B * Hq * (128 + 2) * 4
    if splits > 1 and workspace_bytes is not None and workspace_bytes < per * splits:
        splits = max(workspace_bytes // per, 1)
    return splits


def decode_chunk(T, splits):
    """rows per split, dealt in the kernel from the length the device reads (16-row granularity)"""
    return ((T + splits - 1) // splits + 15) & ~15


def decode_depths(T, splits):
    chunk = decode_chunk(T, splits)
    steps = (chunk + 15) // 16
    return 2 * steps + 4 + 4 + splits + 2, steps + 5


def prefill_depths(kv_len):
    ntiles = (kv_len + 63) // 64
    return 67 * ntiles, ntiles + 1


# ------------------------------------------------------------------ reference

def _as_rows(q):
    return q[:, None] if q.dim() == 3 else q


def reference(q, k, v, pos, scale=None, softcap=0.0, alibi=None, drop=None, with_terms=False):
    """q [B, R, Hq, D] (or [B, Hq, D]: R = 1), k / v [B, >= T, Hkv, D], pos [B, R] (or [B]) integer: query (b, r) sees rows
    t <= pos[b, r].  alibi [Hq] slopes; drop [B, R, Hq] row to leave out of that query's softmax (-1: none).  Everything in float64
    on the inputs' device.  Returns out [B, R, Hq, D] and, with_terms, the per-row tensors the bounds need."""
    q = _as_rows(q).to(torch.float64)
    B, R, Hq, D = q.shape
    dev = q.device
    pos = torch.as_tensor(pos, device=dev).to(torch.int64).reshape(B, -1).expand(B, R)
    T = int(pos.max()) + 1
    k = k[:, :T].to(device=dev, dtype=torch.float64)
    v = v[:, :T].to(device=dev, dtype=torch.float64)
    seen = (torch.arange(T, device=dev).view(1, T) <= pos.amax(1, keepdim=True)).view(B, T, 1, 1)
    k = k.masked_fill(~seen, 0.0)   # rows past every query's position (poisoned in some tests) take no part, not even as 0 * NaN
    v = v.masked_fill(~seen, 0.0)
    Hkv = k.shape[2]
    G = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    kh, vh = k.transpose(1, 2), v.transpose(1, 2)                                     # [B, Hkv, T, D]
    qh = q.permute(0, 2, 1, 3).reshape(B, Hkv, G * R, D)                              # [B, Hkv, G*R, D]: head hk*G + g, row r
    raw = (qh @ kh.transpose(-1, -2) * scale).reshape(B, Hq, R, T)
    t = torch.arange(T, device=dev, dtype=torch.float64)
    mask = t.view(1, 1, T) <= pos.view(B, R, 1).to(torch.float64)                  # [B, R, T]
    mask = mask[:, None].expand(B, Hq, R, T)
    if drop is not None:
        drop = torch.as_tensor(drop, device=dev).to(torch.int64).reshape(B, R, Hq).permute(0, 2, 1)
        mask = mask & (t.view(1, 1, 1, T) != drop[..., None].to(torch.float64))
    capped = softcap * torch.tanh(raw / softcap) if softcap else raw
    bias = None
    if alibi is not None:
        sl = torch.as_tensor(alibi, device=dev).to(torch.float64).view(1, Hq, 1, 1)
        bias = sl * (t.view(1, 1, 1, T) - pos.to(torch.float64).view(B, 1, R, 1))
        s = capped + bias
    else:
        s = capped
    s = s.masked_fill(~mask, float("-inf"))
    M = s.amax(-1, keepdim=True)
    p = torch.exp(s - M).masked_fill(~mask, 0.0)
    sp = p.sum(-1, keepdim=True)
    out = (p.reshape(B, Hkv, G * R, T) @ vh).reshape(B, Hq, R, D) / sp
    res = {"out": out.permute(0, 2, 1, 3).contiguous()}
    if with_terms:
        absqk = (qh.abs() @ kh.abs().transpose(-1, -2) * scale).reshape(B, Hq, R, T)
        mods = None
        if softcap or alibi is not None:
            mods = raw.abs() + s.masked_fill(~mask, 0.0).abs()
            if softcap:
                mods = mods + capped.abs()
            if bias is not None:
                mods = mods + bias.abs()
        res.update(p=p, sp=sp, s=s, M=M, mask=mask, absqk=absqk, mods=mods, out_h=out, vh=vh, G=G)
    return res


def _bound(r, n_dot, depth, n_exp, prefill):
    p, sp, out = r["p"], r["sp"], r["out_h"]                                          # [B, Hq, R, T], [B, Hq, R, 1], [B, Hq, R, D]
    B, Hq, R, T = p.shape
    Hkv = Hq // r["G"]
    gap = (r["M"] - r["s"]).masked_fill(~r["mask"], 0.0)
    eps = gamma(n_dot) * r["absqk"] + 4 * U * torch.as_tensor(n_exp, device=p.device, dtype=torch.float64).view(-1, 1, 1, 1) + 4 * U * gap
    if r["mods"] is not None:
        eps = eps + 8 * U * r["mods"]
    w = p * eps
    if prefill:
        w = w + p * 2.0 ** -11 + 2.0 ** -25 * r["mask"].to(torch.float64)
    absv = r["vh"].abs()
    wv = (w.reshape(B, Hkv, -1, T) @ absv).reshape(B, Hq, R, -1)
    pv = (p.reshape(B, Hkv, -1, T) @ absv).reshape(B, Hq, R, -1)
    acc = 2 * gamma(torch.as_tensor(depth, device=p.device, dtype=torch.float64).view(-1, 1, 1, 1))
    terms = (wv + out.abs() * w.sum(-1, keepdim=True)) / sp + acc * pv / sp + 4 * U * out.abs()
    bound = ulp16(out) + 1.01 * terms
    return bound.permute(0, 2, 1, 3).contiguous()


def _chunked(q, k, v, pos, scale, softcap, alibi, drop, fn):
    """run `fn` on groups of KV heads so that the [B, Hq, R, T] float64 tensors stay below ~2^26 elements each"""
    q = _as_rows(q)
    B, R, Hq, _ = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    T = int(torch.as_tensor(pos).max()) + 1
    per = max(1, (1 << 26) // max(1, B * G * R * T))
    outs, bounds = [], []
    for h0 in range(0, Hkv, per):
        h1 = min(Hkv, h0 + per)
        qs = q[:, :, h0 * G:h1 * G]
        al = None if alibi is None else torch.as_tensor(alibi)[h0 * G:h1 * G]
        dr = None if drop is None else torch.as_tensor(drop).reshape(B, R, Hq)[:, :, h0 * G:h1 * G]
        r = reference(qs, k[:, :, h0:h1], v[:, :, h0:h1], pos, scale, softcap, al, dr, with_terms=True)
        outs.append(r["out"])
        bounds.append(fn(r))
    return torch.cat(outs, 2), torch.cat(bounds, 2)


def decode_bound(q, k, v, lens, splits, scale=None, softcap=0.0, alibi=None, drop=None):
    """Decode class.  q [B, Hq, D], caches [B, Tmax, Hkv, D] (fp16 values or the dequantised fp8 values), lens [B] the number of
    rows each sequence attends over (FUSED: position + 1), `splits` the launch's split count (decode_splits).
    Returns (want, bound), both [B, Hq, D] float64."""
    lens = torch.as_tensor(lens).to(torch.int64).reshape(-1)
    depth, n_exp = zip(*(decode_depths(int(L), splits) for L in lens.tolist()))
    fn = lambda r: _bound(r, DECODE_N_DOT, list(depth), list(n_exp), prefill=False)  # noqa: E731
    want, bound = _chunked(q, k, v, (lens - 1).reshape(-1, 1), scale, softcap, alibi,
                           None if drop is None else torch.as_tensor(drop).reshape(len(lens), 1, -1), fn)
    return want[:, 0], bound[:, 0]


def prefill_bound(q, k, v, start, scale=None, softcap=0.0, alibi=None, drop=None):
    """Prefill class.  q [B, S, Hq, D], caches [>= B, >= start + S, Hkv, D]: query s sees rows <= start + s.
    Returns (want, bound), both [B, S, Hq, D] float64."""
    B, S = q.shape[0], q.shape[1]
    pos = (start + torch.arange(S)).view(1, S).expand(B, S)
    depth, n_exp = prefill_depths(start + S)
    fn = lambda r: _bound(r, PREFILL_N_DOT, depth, n_exp, prefill=True)  # noqa: E731
    return _chunked(q, k[:B], v[:B], pos, scale, softcap, alibi, drop, fn)


def assert_attention_close(got, want, bound, what=""):
    """|got - want| <= bound element by element (NaN fails).  The message names the count, the worst element by error / bound
    (batch, [row,] head, dim) and that ratio."""
    got = torch.as_tensor(got).to(torch.float64)
    want = torch.as_tensor(want).to(device=got.device, dtype=torch.float64)
    bound = torch.as_tensor(bound).to(device=got.device, dtype=torch.float64)
    err = (got - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bound)
        i = int(torch.argmax(ratio))
        idx = tuple(int(x) for x in np.unravel_index(i, tuple(err.shape)))
        names = ("batch", "head", "dim") if err.dim() == 3 else ("batch", "row", "head", "dim")
        at = ", ".join(f"{n} {x}" for n, x in zip(names, idx))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the attention bound; worst at ({at}): "
                             f"got {float(got[idx]):.6g}, want {float(want[idx]):.6g}, error {float(err[idx]):.3g} = "
                             f"{float(ratio[idx]):.3g} x the bound {float(bound[idx]):.3g}")


def worst_ratio(got, want, bound):
    got = torch.as_tensor(got).to(torch.float64)
    err = (got - torch.as_tensor(want).to(device=got.device, dtype=torch.float64)).abs()
    return float((err / torch.as_tensor(bound).to(device=got.device, dtype=torch.float64)).max())


def needle_margin(want, want_without, bound):
    """how far the reference without the target row lies from the reference, in units of the bound: per (b, [row,] head),
    the largest |want - want_without| / bound over the head dimension"""
    return ((want - want_without).abs() / bound).amax(-1)


def target_weight(q, k, v, pos, target, scale=None, softcap=0.0, alibi=None):
    """softmax weight of row target[b, r, h] in query (b, r, h)'s softmax -> [B, R, Hq]"""
    r = reference(q, k, v, pos, scale, softcap, alibi, with_terms=True)
    p, sp = r["p"], r["sp"]
    B, Hq, R, T = p.shape
    tg = torch.as_tensor(target, device=p.device).to(torch.int64).reshape(B, R, Hq).permute(0, 2, 1)
    w = torch.gather(p, -1, tg[..., None].clamp(0, T - 1))[..., 0] / sp[..., 0]
    return w.permute(0, 2, 1)
