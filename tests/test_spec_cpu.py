"""Speculative decoding without a GPU: the ABI of the new entry points, and the property that makes the feature safe -- the
speculative loop built from spec_ref.accept / spec_ref.draft emits exactly the plain greedy loop's tokens."""
import ctypes

import numpy as np
import pytest

import spec_ref


def test_abi_symbols_exist():
    from autoawq_amd import _lib

    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("awq_verify_attention_rows", "awq_verify_attention_workspace_bytes", "awq_verify_attention_splits",
                 "awq_spec_accept", "awq_ngram_draft"):
        assert hasattr(h, name), name
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.AwqSpecParams) == 48 and ctypes.sizeof(_lib.AwqSpecArgs) == 144
    lib = _lib.lib()
    assert lib.awq_verify_attention_workspace_bytes(2, 4, 8) == 2 * 4 * 8 * 64 * 130 * 4
    # the decode launch's split rule with the token groups counted as blocks: G = 8 -> T groups of one token
    assert lib.awq_verify_attention_splits(256, 1, 4, 8, 1) == 1
    assert lib.awq_verify_attention_splits(257, 1, 4, 8, 1) == 3
    assert lib.awq_verify_attention_splits(4096, 4, 8, 32, 32) == 1024 // (4 * 32 * 1)
    assert lib.awq_verify_attention_splits(4096, 4, 8, 32, 4) == 1024 // (4 * 4 * 8)


def _toy(seed, vocab=5, ctx=2):
    """next token = a hash of the last `ctx` tokens into a small vocabulary, so that the text soon repeats"""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, vocab, size=(vocab,) * ctx)

    def f(prefix):
        key = tuple(int(x) for x in prefix[-ctx:])
        key = (0,) * (ctx - len(key)) + key
        return int(table[key])
    return f, rng


@pytest.mark.parametrize("T", range(2, 9))
@pytest.mark.parametrize("ngram_max", [1, 2, 3])
def test_speculative_loop_equals_plain_greedy(T, ngram_max):
    best = 0
    for seed in range(40):
        f, rng = _toy(seed)
        prompt = [int(x) for x in rng.integers(0, 5, size=int(rng.integers(1, 9)))]
        for eos, budget in (((), 37), ((3,), 37), ((), 5), ((1, 4), 11)):   # 37, 5, 11: budgets that end inside a step
            want = spec_ref.greedy_loop(f, prompt, budget, eos)
            got, per_step = spec_ref.spec_loop(f, prompt, budget, T, ngram_max, eos)
            assert got == want, (seed, eos, budget)
            assert len(got) <= budget and all(1 <= m <= T for m in per_step)
            best = max([best] + per_step)
    assert best > 1, "no step accepted a draft: the property above would be vacuous"


def test_draft_cases():
    d = spec_ref.draft
    assert d([7], 4, 3) == [7, 7, 7, 7]                                   # n = 1: nothing to match
    assert d([1, 2, 3, 4], 3, 3) == [4, 4, 4]                             # no match: fillers
    assert d([1, 2, 3, 9, 1, 2, 3], 4, 3) == [3, 9, 1, 2]                 # match at index 0
    assert d([5, 1, 2, 8, 1, 2], 5, 2) == [2, 8, 1, 2, 2]                 # the continuation runs into the end: filler
    assert d([1, 2, 7, 1, 2, 8, 1, 2], 3, 2) == [2, 8, 1]                 # the LARGEST s wins
    assert d([3, 1, 9, 2, 1], 3, 3) == [1, 9, 2]                          # falls back to g = 1
    assert d([4, 4, 4], 3, 2) == [4, 4, 4]                                # overlapping match, s = n - g - 1


def test_accept_cases():
    a = spec_ref.accept
    assert a([9, 1, 2, 3], [1, 2, 3, 4], 1, 100) == ([1, 2, 3, 4], False)   # every draft accepted: T tokens
    assert a([9, 1, 5, 3], [1, 2, 3, 4], 1, 100) == ([1, 2], False)         # the first mismatch ends the run, its argmax is kept
    assert a([9, 8, 2, 3], [1, 2, 3, 4], 1, 100) == ([1], False)
    assert a([9, 1, 2, 3], [1, 2, 3, 4], 1, 100, (2,)) == ([1, 2], True)    # EOS inside the accepted run, inclusive
    assert a([9, 1, 2, 3], [1, 2, 3, 4], 98, 100) == ([1, 2], True)         # the budget ends inside it
    assert a([9, 1, 2, 3], [1, 2, 3, 4], 1, 100, (4,)) == ([1, 2, 3, 4], True)
