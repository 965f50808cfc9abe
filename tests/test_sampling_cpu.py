"""CPU checks of the token-selection contract (csrc/sample.hip): the Philox restatement against numpy's generator, the kept
sets against transformers' warpers, the documented tie rules, and argument validation before any device call."""
import numpy as np
import pytest
import torch

import sampling_ref as ref


@pytest.mark.parametrize("seed,t,row,block", [(0, 1, 0, 0), (123, 5, 3, 7), (2 ** 63 + 5, 99, 1023, 38015), (7, 2 ** 40, 1, 3)])
def test_philox_restatement_equals_numpy(seed, t, row, block):
    want = np.random.Philox(key=np.array([seed, 0], dtype=np.uint64),
                            counter=np.array([t - 1, row, block, 0], dtype=np.uint64)).random_raw(4)
    got = ref.philox4x64_10((np.uint64(t), np.uint64(row), np.uint64(block), np.uint64(0)), (np.uint64(seed), np.uint64(0)))
    assert [int(x) for x in got] == [int(x) for x in want]


def test_uniforms_in_open_unit_interval_and_word_mapping():
    u = ref.uniforms(3, 2, 1, 10)
    assert u.dtype == np.float32 and ((u > 0) & (u < 1)).all()
    w = np.random.Philox(key=np.array([3, 0], dtype=np.uint64), counter=np.array([1, 1, 2, 0], dtype=np.uint64)).random_raw(4)
    for j in (0, 1):
        assert u[8 + j] == np.float32((np.float32(int(w[j]) >> 41) + np.float32(0.5)) * np.float32(2.0 ** -23))


def test_extreme_words_give_finite_gumbel_terms():
    """The largest and smallest Philox words: u stays strictly inside (0, 1) in fp32, so -log(-log(u)) is finite (the 24-bit form
    ((w >> 40) + 0.5) * 2^-24 rounds to exactly 1.0 for the largest word: an infinite term that wins whatever the logit)."""
    words = np.array([2 ** 64 - 1, 2 ** 64 - 2 ** 41, 2 ** 41 - 1, 0], dtype=np.uint64)
    u = ref.uniform_of_word(words)
    assert (u < np.float32(1.0)).all() and (u > 0).all()
    assert u[0] == np.float32(1.0) - np.float32(2.0 ** -24) and u[-1] == np.float32(2.0 ** -24)
    g = -np.log(-np.log(u.astype(np.float32)))  # fp32, as the kernel evaluates it
    assert np.isfinite(g).all()
    old = ((words >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert old[0] == np.float32(1.0)  # the flaw the 23-bit form removes


def _hf_kept(v, temperature, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    s = torch.from_numpy(v.astype(np.float64))[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    s = TemperatureLogitsWarper(temperature)(ids, s)
    if top_k:
        s = TopKLogitsWarper(top_k)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p)(ids, s)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("case", range(40))
def test_kept_sets_equal_transformers_warpers_on_tie_free_logits(case):
    rng = np.random.default_rng(case)
    V = int(rng.integers(8, 400))
    v = rng.permutation(np.unique((rng.standard_normal(4 * V) * 2).astype(np.float16)))[:V].astype(np.float64)
    V = len(v)
    temperature = float(rng.choice([0.5, 0.8, 1.0, 1.7]))
    top_k = int(rng.choice([0, 1, 5, V // 2, V]))
    top_p = float(rng.choice([1.0, 0.95, 0.9, 0.5, 0.1]))
    got = ref.kept_set(v, temperature, top_k, top_p)
    assert np.array_equal(got, _hf_kept(v, temperature, top_k, top_p)), (V, temperature, top_k, top_p)


def test_tie_rules():
    v = np.array([1.0, 3.0, 3.0, 3.0, 0.0, -np.inf, 3.0])
    # top-k: every token equal to the k-th largest is kept
    assert ref.kept_set(v, 1.0, 2, 1.0).tolist() == [False, True, True, True, False, False, True]
    # top-p: a tied group at the threshold is kept whole (the four 3.0 carry ~0.98 together)
    assert ref.kept_set(v, 1.0, 0, 0.3).tolist() == [False, True, True, True, False, False, True]
    # -inf never kept, even with everything else off
    assert not ref.kept_set(v, 1.0, 0, 1.0)[5]
    # greedy: the lowest index of the maximum (torch.argmax's rule); -0 and +0 are equal
    assert ref.choose(v, do_sample=False)[0] == 1
    assert ref.choose(np.array([-0.0, 0.0, -1.0]), do_sample=False)[0] == 0
    assert int(torch.argmax(torch.tensor([1.0, 3.0, 3.0]))) == 1
    # bad rows
    assert ref.choose(np.array([1.0, np.nan]), do_sample=False)[0] is None
    assert ref.choose(np.array([1.0, np.inf]), do_sample=True)[0] is None
    assert ref.choose(np.array([-np.inf, -np.inf]), do_sample=True)[0] is None


def test_gumbel_max_draws_follow_the_probabilities():
    v = np.array([0.0, 1.0, 2.0, -1.0, 0.5, 1.5, -np.inf, 0.2])
    p = ref.probabilities(v, 1.0, 0, 1.0)
    counts = np.zeros(len(v))
    for t in range(1, 4001):
        counts[ref.choose(v, do_sample=True, seed=1, t=t)[0]] += 1
    assert counts[6] == 0
    e = 4000 * p[p > 0]
    assert (((counts[p > 0] - e) ** 2) / e).sum() < 30.0


def test_sample_tokens_validates_before_any_device_call():
    from autoawq_amd import ops

    x = torch.zeros((2, 16), dtype=torch.float16)  # a CPU tensor: a device call would raise AwqHipError, not ValueError
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=True, top_p=0.0)
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=True, top_p=1.5)
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=True, top_k=-1)
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=True, eos_ids=list(range(9)))
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=False, t=0)


def test_sample_params_layout():
    from autoawq_amd import _lib, ops

    import ctypes

    assert ctypes.sizeof(_lib.AwqSampleParams) == 64
    b = ops.sample_params(do_sample=True, temperature=0.5, top_k=7, top_p=0.9, seed=2 ** 64 - 1, eos_ids=[3, 4])
    p = _lib.AwqSampleParams.from_buffer_copy(bytes(b.numpy()))
    assert (p.seed, p.do_sample, p.top_k, p.n_eos, p.pad, list(p.eos)[:2]) == (2 ** 64 - 1, 1, 7, 2, 3, [3, 4])
    assert abs(p.temperature - 0.5) < 1e-7 and abs(p.top_p - 0.9) < 1e-7
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    assert callable(GraphedDecoder.generate)
