"""fp64 numpy restatement of the token-selection contract of csrc/sample.hip (see its header comment), the oracle of
tests/test_sampling_cpu.py and tests/test_gpu_sampling.py.  Vectorised Philox4x64-10 (checked against np.random.Philox)."""
import numpy as np

M0, M1 = np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157)
W0, W1 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    a0, a1 = a & _LO, a >> _S32
    b0, b1 = b & _LO, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _LO) + (p10 & _LO)
    return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32), a * b


def philox4x64_10(ctr, key):
    """ctr: four uint64 arrays (broadcastable), key: two uint64 -> the four output words (Random123's rounds and key bumps)."""
    with np.errstate(over="ignore"):
        c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in ctr])]
        k0, k1 = np.uint64(key[0]), np.uint64(key[1])
        for r in range(10):
            if r:
                k0, k1 = k0 + W0, k1 + W1
            hi0, lo0 = _mulhilo(M0, c[0])
            hi1, lo1 = _mulhilo(M1, c[2])
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def uniforms(seed, t, row, V):
    """u_i, i < V, as the kernel forms them: fp32 ((w >> 41) + 0.5) * 2^-23 -- exact, so 0 < u < 1."""
    blocks = np.arange((V + 3) // 4, dtype=np.uint64)
    w = philox4x64_10((np.uint64(t), np.uint64(row), blocks, np.uint64(0)), (np.uint64(seed), np.uint64(0)))
    words = np.stack(w, axis=1).reshape(-1)[:V]
    return uniform_of_word(words)


def uniform_of_word(words):
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(41)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def gumbel(seed, t, row, V):
    u = uniforms(seed, t, row, V).astype(np.float64)
    return -np.log(-np.log(u))


def bad_row(logits):
    v = np.asarray(logits, dtype=np.float64)
    return bool(np.isnan(v).any() or np.isposinf(v).any())


def kept_set(logits, temperature=1.0, top_k=0, top_p=1.0):
    """Boolean mask of the tokens that survive temperature -> top-k -> top-p (the contract's tie rules)."""
    v = np.asarray(logits, dtype=np.float64)
    keep = ~np.isneginf(v)
    if not keep.any():
        return keep
    x = v / temperature
    if 0 < top_k < keep.sum():
        kth = np.sort(x[keep])[-top_k]
        keep &= x >= kth
    if top_p < 1.0:
        m = np.where(keep, np.exp(x - x[keep].max()), 0.0)
        z = m.sum()
        vals = np.unique(x[keep])[::-1]  # distinct kept values, descending
        mass = np.array([m[x >= tau].sum() for tau in vals]) if len(vals) < 4096 else np.cumsum([m[x == tau].sum() for tau in vals])
        tau = vals[np.argmax(mass >= top_p * z)]
        keep &= x >= tau
    return keep


def scores(logits, seed, t, row, temperature=1.0):
    v = np.asarray(logits, dtype=np.float64)
    return v / temperature + gumbel(seed, t, row, len(v))


def choose(logits, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0, t=1, row=0):
    """(token, kept mask, scores or None); token None for a bad row or an empty kept set."""
    v = np.asarray(logits, dtype=np.float64)
    if bad_row(v) or np.isneginf(v).all():
        return None, None, None
    if not do_sample or temperature <= 0:
        return int(np.argmax(v)), None, None
    keep = kept_set(v, temperature, top_k, top_p)
    s = np.where(keep, scores(v, seed, t, row, temperature), -np.inf)
    return int(np.argmax(s)), keep, s


def probabilities(logits, temperature=1.0, top_k=0, top_p=1.0):
    v = np.asarray(logits, dtype=np.float64)
    keep = kept_set(v, temperature, top_k, top_p)
    x = np.where(keep, v / temperature, -np.inf)
    p = np.exp(x - x.max())
    return p / p.sum()
