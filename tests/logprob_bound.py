"""fp64 reference for awq_token_logprobs (csrc/logprob.hip) and a per-element error bound derived from the kernel's arithmetic.

`reference(x, ids)` is (x[id] - m) - log sum_i exp(x_i - m) in numpy float64 on the fp16 logits, with the contract's special
cases (id < 0: 0.0; id >= V, a row holding NaN or +inf, a row of nothing but -inf: NaN; the id's own logit -inf: -inf).
`logprob_bound` returns it with the bound beside it, `assert_logprobs_close` compares a kernel's output with both, `emulate`
restates the kernel's order of operations in numpy float32.

Notation: u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u), m = max_i x_i, g_i = m - x_i >= 0, p_i = exp(-g_i),
S = sum_i p_i (1 <= S <= V), L = log S, y = (x_id - m) - L the exact result.

The kernel (restated from the header of csrc/logprob.hip)
---------------------------------------------------------
1024 threads per row, 8 halves per thread per step, steps = ceil(V / 8192).  The fp16 logits are exact in fp32, and so is every
maximum.  A thread keeps a running (m_t, s_t): per 8-vector one rescale s_t *= exp(m_old - m_new) when the maximum grows, then
eight sequential adds of exp(x_j - m_t).  Two partials merge as s = s_a e_a + s_b e_b, e = exp(m_side - max) (exactly 1 on the
side that holds the maximum): 6 levels inside a wave, 4 levels over the 16 waves.  Thread 0 returns (x_id - m) - logf(S~).

    N(V)     = 9 steps + 2 (6 + 4) = 9 steps + 20     adds and rescale multiplies on one term's path into S~
    n_exp(V) = 1 + steps + 6 + 4   = steps + 11       exp evaluations on one term's chain: its own, <= 1 rescale per step, 1 per merge

The bound
---------
S~ = sum p~_i with p~_i = p_i (1 + eps_i) summed in fp32.  dy = -dS / S to first order, so

    |y~ - y| <= 1.01 * [ sum_i p_i (4 u n_exp + 4 u g_i) / S      (the weights: exp errors, below)
                         + gamma(N)                               (fp32 accumulation: gamma(N) sum p_i / S)
                         + 4 u |L|                                (logf: within 2 ulp of log S~)
                         + 2 u |x_id - m| ]                       (the rounding of x_id - m, taken twice)
                 + 2 u |y|                                        (the final subtraction, taken twice)

1.01 covers the second-order products (every first-order term is < 1e-2 here).

eps_i: every exp on a term's chain is v_exp_f32 (<= 1 ulp; taken as 2 ulp = 4 u) -- at most n_exp of them: 4 u n_exp.  The kernel
works in the log2 domain: exp(a) = v_exp_f32(fl(a * fl(log2 e))) with a = fl(x - m') itself a rounded difference.  That is three
relative perturbations of at most u on the argument (the difference, the rounded constant, the product), each moving the result by
the factor e^(u |a|).  The arguments of one term's chain telescope -- (m_1 - x_i) + (m_2 - m_1) + ... = m - x_i = g_i, all of one
sign -- so together they contribute 3 u g_i, inside the 4 u g_i the bound grants (the same allowance tests/attn_bound.py makes for
a once- or twice-rounded argument).  Terms whose fp32 p underflows (g_i > 87) are off by < 2^-126 relative to the maximum's 1.

With p_i = 0 (x_i = -inf) a term contributes nothing.  The bound at V = 32000 is about 1e-5 .. 6e-5 absolute.
"""
import numpy as np

U = 2.0 ** -24
THREADS, VEC = 1024, 8
STEP = THREADS * VEC      # elements per step: the kernel's per-step width
WAVE = 64


def gamma(n):
    return n * U / (1.0 - n * U)


def steps(V):
    return (int(V) + STEP - 1) // STEP


def depths(V):
    """(summation depth N, exp evaluations per term n_exp) of the kernel at vocabulary V"""
    return 9 * steps(V) + 20, steps(V) + 11


def _rows(x, ids):
    x = np.asarray(x)
    ids = np.asarray(ids, np.int64)
    if x.ndim == 1:
        x = x[None]
    ids = ids.reshape(-1)
    assert x.dtype == np.float16 and x.ndim == 2 and ids.shape[0] == x.shape[0], (x.dtype, x.shape, ids.shape)
    return x, ids


def logprob_bound(x, ids, drop=None):
    """x fp16 [R, V] (or [V]), ids int64 [R]; drop [R]: an index left out of that row's softmax (-1: none).
    Returns (want, bound), float64 [R]: the contract's answer and the bound on |kernel - want| (0 where the answer is exact by
    contract: NaN, -inf, an ignored slot)."""
    x, ids = _rows(x, ids)
    R, V = x.shape
    N, n_exp = depths(V)
    want, bound = np.zeros(R), np.zeros(R)
    for r in range(R):
        i = int(ids[r])
        if i < 0:
            continue
        row = x[r].astype(np.float64)
        if drop is not None and int(drop[r]) >= 0:
            row = np.delete(row, int(drop[r]))
            assert i != int(drop[r])
            i -= i > int(drop[r])
        m = row.max() if not np.isnan(row).any() else np.nan
        if i >= V or not m < np.inf or m == -np.inf:   # id out of range, NaN / +inf in the row, nothing but -inf
            want[r] = np.nan
            continue
        if row[i] == -np.inf:
            want[r] = -np.inf
            continue
        live = row > -np.inf
        g = m - row[live]
        p = np.exp(-g)
        S = p.sum()
        L = np.log(S)
        d = row[i] - m
        y = d - L
        want[r] = y
        bound[r] = 1.01 * ((p * (4 * U * n_exp + 4 * U * g)).sum() / S + gamma(N) + 4 * U * abs(L) + 2 * U * abs(d)) + 2 * U * abs(y)
    return want, bound


def reference(x, ids):
    return logprob_bound(x, ids)[0]


def check(got, want, bound):
    """-> (ok [R] bool, ratio [R]): NaN is required where the contract says NaN and fails elsewhere; an infinite answer must be
    met exactly; every other element within the bound (no extra factor)."""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    bound = np.asarray(bound, np.float64).reshape(-1)
    exact = ~np.isfinite(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ok = np.where(np.isnan(want), np.isnan(got), np.where(exact, got == want, err <= bound))
        ratio = np.where(exact | (bound == 0), np.where(ok, 0.0, np.inf), err / np.where(bound == 0, 1.0, bound))
    return ok, np.where(np.isnan(ratio), np.inf, ratio)


def assert_logprobs_close(got, want, bound, what=""):
    ok, ratio = check(got, want, bound)
    if not ok.all():
        i = int(np.argmax(ratio))
        g, w = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
        raise AssertionError(f"{what}: {int((~ok).sum())}/{ok.size} rows outside the log-prob bound; worst row {i}: got {g[i]!r}, "
                             f"want {w[i]!r}, {ratio[i]:.3g} x the bound {np.asarray(bound).reshape(-1)[i]:.3g}")
    return float(ratio.max()) if ratio.size else 0.0


def needle_margin(want, want_without, bound):
    """how far the reference without the needle lies from the reference, in units of the bound"""
    return np.abs(np.asarray(want) - np.asarray(want_without)) / np.asarray(bound)


# ---------------------------------------------------------------- the kernel's order of operations, in numpy float32

_LOG2E = np.float32(1.4426950408889634)


def _exp32(a):
    """exp as the kernel takes it: 2^(fl(a * fl(log2 e))), the power itself correctly rounded here (the hardware's is within an ulp)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp2((a.astype(np.float32) * _LOG2E).astype(np.float64)).astype(np.float32)


def _merge(m, s, mo, so):
    with np.errstate(invalid="ignore"):
        M = np.maximum(m, mo)
        ea = np.where(m == M, np.float32(1), _exp32(m - M))
        eb = np.where(mo == M, np.float32(1), _exp32(mo - M))
        out = (s * ea).astype(np.float32) + (so * eb).astype(np.float32)
    return M, np.where(M == -np.inf, s, out).astype(np.float32)


def owner(e, vec=True):
    """(step, thread, slot) of element e: who adds it, and when"""
    k, o = divmod(int(e), STEP)
    return (k, o // VEC, o % VEC) if vec else (k, o % THREADS, o // THREADS)


def emulate(row, i, vec=True):
    """One finite-or--inf row (fp16 [V]) and an id in [0, V) through the kernel's arithmetic in float32.  vec: the 16-byte path
    (thread t of step k owns elements 8192 k + 8 t ..), else the element path (8192 k + 1024 j + t)."""
    row = np.asarray(row, np.float16)
    V = row.shape[0]
    n = steps(V)
    x = np.full(n * STEP, -np.inf, np.float32)
    x[:V] = row.astype(np.float32)
    x = x.reshape(n, THREADS, VEC) if vec else x.reshape(n, VEC, THREADS).transpose(0, 2, 1)
    m = np.full(THREADS, -np.inf, np.float32)
    s = np.zeros(THREADS, np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(n):
            v = x[k].max(1)
            up = v > m
            s = np.where(up, (s * _exp32(m - v)).astype(np.float32), s)
            m = np.where(up, v, m)
            live = m > -np.inf
            for j in range(VEC):
                s = np.where(live, (s + _exp32(x[k][:, j] - m)).astype(np.float32), s)
        idx = np.arange(THREADS)
        d = 1
        while d < WAVE:
            m, s = _merge(m, s, m[idx ^ d], s[idx ^ d])
            d *= 2
        m, s = m[::WAVE].copy(), s[::WAVE].copy()
        idx = np.arange(THREADS // WAVE)
        d = 1
        while d < THREADS // WAVE:
            m, s = _merge(m, s, m[idx ^ d], s[idx ^ d])
            d *= 2
    if m[0] == -np.inf:
        return np.float32(np.nan)
    with np.errstate(divide="ignore"):
        return np.float32(np.float32(np.float32(row[i]) - m[0]) - np.float32(np.log(np.float64(s[0]))))


# ---------------------------------------------------------------- the row kinds the tests share

KINDS = ("normal", "ascending", "descending", "flat", "high", "low", "sparse")


def make_row(kind, V, rng):
    """fp16 [V].  ascending: every step rescales; high / low: values around +-60000; sparse: 90 % -inf."""
    if kind == "normal":
        x = rng.standard_normal(V) * 3.0
    elif kind == "ascending":
        x = np.linspace(-8.0, 8.0, V) if V > 1 else np.array([0.5])
    elif kind == "descending":
        x = np.linspace(8.0, -8.0, V) if V > 1 else np.array([0.5])
    elif kind == "flat":
        x = np.full(V, 1.25)
    elif kind == "high":
        x = 60000.0 + rng.standard_normal(V) * 64.0
    elif kind == "low":
        x = -60000.0 + rng.standard_normal(V) * 64.0
    elif kind == "sparse":
        x = rng.standard_normal(V) * 3.0
        x[rng.random(V) < 0.9] = -np.inf
        x[int(rng.integers(V))] = 2.0   # at least one finite logit
    else:
        raise ValueError(kind)
    return np.clip(x, -65504.0, 65504.0).astype(np.float16) if kind != "sparse" else x.astype(np.float16)


def targets(row):
    """the ids every row is scored at: 0, V // 2, V - 1 and the row's argmax"""
    V = row.shape[0]
    return sorted({0, V // 2, V - 1, int(np.argmax(row.astype(np.float32)))})
