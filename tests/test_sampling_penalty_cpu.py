"""CPU checks of the sampler's logit processors (csrc/sample.hip, awq_sample_tokens_ex): the numpy restatement
tests/penalty_ref.py against transformers' RepetitionPenaltyLogitsProcessor -> MinNewTokensLengthLogitsProcessor, the pinned
saturation cases, the whole processors + warpers pipeline on tie-free rows, argument validation before any device call, and the
ctypes structs against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import penalty_ref as pref
import sampling_ref as ref
from conftest import ROOT

PENALTIES = [0.5, 1.0, 1.05, 1.3, 2.0]


def _row(rng, V):
    """fp16 logits with negatives, +-0, -inf and the odd +inf"""
    x = (rng.standard_normal(V) * rng.choice([1.0, 4.0, 3000.0])).astype(np.float16)
    x[rng.integers(0, V, 3)] = np.float16(0.0)
    x[rng.integers(0, V, 3)] = np.float16(-0.0)
    x[rng.integers(0, V, 4)] = np.float16(-np.inf)
    if rng.random() < 0.3:
        x[rng.integers(0, V)] = np.float16(np.inf)
    return x


def _hf_processed(x, input_ids, prompt_len, p, min_new, eos):
    """transformers' processors on the fp32 cast of the fp16 logits, as `generate` runs them: fp32 [V]"""
    from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor

    ids = torch.tensor(np.asarray(input_ids, dtype=np.int64))[None]
    s = torch.from_numpy(x.astype(np.float32))[None]
    if p != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=p)(ids, s)
    if min_new > 0 and len(eos):
        s = MinNewTokensLengthLogitsProcessor(prompt_len, min_new, list(eos))(ids, s)
    return s[0].numpy()


def _case(seed):
    rng = np.random.default_rng(seed)
    V = int(rng.integers(16, 600))
    x = _row(rng, V)
    prompt_len = int(rng.integers(1, 40))
    min_new = int(rng.integers(0, 6))
    t = max(1, min_new + int(rng.integers(-2, 3)))          # around min_new_tokens
    hi = int(rng.integers(4, V + 1))                          # a small id range: duplicates are common
    input_ids = rng.integers(0, hi, prompt_len + t - 1)
    eos = sorted(set(int(e) for e in rng.integers(0, V, int(rng.integers(1, 4)))))
    return rng, V, x, prompt_len, min_new, t, input_ids, eos


@pytest.mark.parametrize("p", PENALTIES)
@pytest.mark.parametrize("seed", range(24))
def test_process_equals_transformers_processors(seed, p):
    rng, V, x, prompt_len, min_new, t, input_ids, eos = _case(seed)
    hf = _hf_processed(x, input_ids, prompt_len, p, min_new, eos)
    seen = pref.seen_mask(pref.bitmap([input_ids], V)[0], V)
    got = pref.process(x, seen, t=t, repetition_penalty=p, min_new_tokens=min_new, eos_ids=eos)
    assert got.dtype == np.float16
    in_range = ~np.isfinite(hf) | (np.abs(hf) <= 65504.0)
    want = hf.astype(np.float16)
    assert np.array_equal(got[in_range].view(np.uint16), want[in_range].view(np.uint16)), seed
    # out of fp16 range (a penalty below 1 on a large logit): saturated, never infinite
    out = ~in_range
    assert np.array_equal(got[out], np.where(hf[out] > 0, np.float16(65504), np.float16(-65504)))
    if t <= min_new:
        assert np.isneginf(got[eos].astype(np.float32)).all()


def test_suppression_window_edges():
    V = 20
    x = np.linspace(-3, 3, V).astype(np.float16)
    seen = np.zeros(V, dtype=bool)
    for t in range(1, 7):
        got = pref.process(x, seen, t=t, min_new_tokens=4, eos_ids=[19, 3])
        assert np.isneginf(got[[19, 3]].astype(np.float32)).all() == (t <= 4)
        assert np.array_equal(np.delete(got, [3, 19]), np.delete(x, [3, 19]))


def test_saturation_cases_pinned():
    x = np.array([65504, -65504, 1.0, -1.0, 0.0, -0.0, -np.inf, np.inf, np.nan], dtype=np.float16)
    seen = np.ones(len(x), dtype=bool)
    half = pref.process(x, seen, repetition_penalty=0.5)
    two = pref.process(x, seen, repetition_penalty=2.0)
    assert half[:6].tolist() == [65504.0, -32752.0, 2.0, -0.5, 0.0, 0.0]
    assert two[:6].tolist() == [32752.0, -65504.0, 0.5, -2.0, 0.0, 0.0]
    assert [np.signbit(v) for v in half[4:6]] == [False, True] and [np.signbit(v) for v in two[4:6]] == [False, True]
    for r in (half, two):   # the non-finite pass unchanged, the finite stay finite: no new status bit
        assert np.isneginf(r[6]) and np.isposinf(r[7]) and np.isnan(r[8])
        assert np.isfinite(r[:6]).all()
        assert not ref.bad_row(r[:7])


def _tie_free(v):
    f = v[np.isfinite(v)]
    return len(np.unique(f)) == len(f)


def _hf_warped_kept(scores, temperature, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    s = torch.from_numpy(np.asarray(scores, dtype=np.float64))[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    s = TemperatureLogitsWarper(temperature)(ids, s)
    if top_k:
        s = TopKLogitsWarper(top_k)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p)(ids, s)
    return torch.isfinite(s[0]).numpy()


def test_choose_of_processed_equals_transformers_pipeline():
    """Greedy: the argmax of transformers' fp32 processed scores.  Sampled: the kept set of transformers' warpers (top-k on the fp32
    scores; with top-p, on the fp16 rounding the contract fixes), and the drawn token inside it.  On the rows that are tie-free
    after processing (the documented tie rule); most of the random rows are."""
    checked = 0
    for seed in range(60):
        rng, V, _, prompt_len, min_new, t, input_ids, eos = _case(1000 + seed)
        x = rng.permutation(np.unique((rng.standard_normal(4 * V) * 3).astype(np.float16)))[:V]
        V = len(x)
        x[rng.integers(0, V, 3)] = np.float16(-np.inf)
        input_ids, eos = input_ids % V, [e % V for e in eos]
        p = float(rng.choice(PENALTIES))
        hf = _hf_processed(x, input_ids, prompt_len, p, min_new, eos)
        seen = pref.seen_mask(pref.bitmap([input_ids], V)[0], V)
        v = pref.process(x, seen, t=t, repetition_penalty=p, min_new_tokens=min_new, eos_ids=eos)
        if not _tie_free(v):
            continue
        checked += 1
        assert ref.choose(v, do_sample=False)[0] == int(np.argmax(hf)), seed
        temperature = float(rng.choice([0.6, 1.0, 1.4]))
        top_k = int(rng.choice([0, 1, 5, V // 3]))
        top_p = float(rng.choice([1.0, 0.9, 0.5]))
        kept = ref.kept_set(v, temperature, top_k, top_p)
        hf_kept = _hf_warped_kept(hf if top_p == 1.0 else hf.astype(np.float16).astype(np.float64), temperature, top_k, top_p)
        assert np.array_equal(kept, hf_kept), seed
        tok, _, _ = ref.choose(v, do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, t=t, row=0)
        assert hf_kept[tok]
    assert checked >= 30, checked


def test_bitmap_layout():
    V = 100
    h = pref.bitmap([[0, 31, 32, 99, 99, -1, 100], []], V).view(np.uint32)
    assert h.shape == (2, 4)
    assert h[0].tolist() == [1 | (1 << 31), 1, 0, 1 << 3] and h[1].tolist() == [0, 0, 0, 0]
    assert np.flatnonzero(pref.seen_mask(h[0], V)).tolist() == [0, 31, 32, 99]


# ---- validation before any device call ------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_proc_params_refuse_bad_penalties(p):
    from autoawq_amd import ops

    with pytest.raises(ValueError):
        ops.sample_proc_params(repetition_penalty=p)


@pytest.mark.parametrize("m", [-1, 1.5, True])
def test_proc_params_refuse_bad_min_new_tokens(m):
    from autoawq_amd import ops

    with pytest.raises(ValueError):
        ops.sample_proc_params(min_new_tokens=m)


def test_proc_params_packing():
    from autoawq_amd import _lib, ops

    b = ops.sample_proc_params(repetition_penalty=1.05, min_new_tokens=8)
    assert b.dtype == torch.uint8 and b.numel() == 16
    q = _lib.AwqSampleProc.from_buffer_copy(bytes(b.numpy()))
    assert q.repetition_penalty == np.float32(1.05) and q.min_new_tokens == 8 and list(q.pad) == [0, 0]
    assert ops.sample_proc_params(min_new_tokens=2 ** 40)[4:8].view(torch.int32).item() == 2 ** 31 - 1


def test_history_validation():
    from autoawq_amd import ops

    with pytest.raises(ValueError):
        ops.sample_history(torch.zeros((1, 4), dtype=torch.int64), 0)
    with pytest.raises(ValueError):
        ops.sample_history(torch.zeros((1, 4), dtype=torch.int64), (1 << 20) + 1)
    with pytest.raises(ValueError):
        ops.sample_history(torch.tensor([[0, 5, 10]]), 10)           # id == vocab
    with pytest.raises(ValueError):
        ops.sample_history(torch.tensor([[-1, 5]]), 10)
    with pytest.raises(ValueError):
        ops.sample_history(torch.zeros((1, 4)), 10)                   # float ids
    with pytest.raises(ValueError):
        ops.sample_history(torch.zeros((2, 4), dtype=torch.int64), 64, out=torch.zeros((2, 1), dtype=torch.int32))
    assert ops.sample_history_words(1) == 1 and ops.sample_history_words(32) == 1 and ops.sample_history_words(152064) == 4752


def test_sample_tokens_penalty_needs_a_history():
    from autoawq_amd import ops

    x = torch.zeros((1, 8), dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=False, repetition_penalty=1.3)
    with pytest.raises(ValueError):
        ops.sample_tokens(x, do_sample=False, repetition_penalty=0.0, history=torch.zeros((1, 1), dtype=torch.int32))


# ---- ABI -----------------------------------------------------------------------------------------------------------------

_CTYPES = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}


def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "awq_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(?:\[(\d+)\])?$", decl)
        assert m, decl
        ty, ptr, fname, n = m.groups()
        c = ctypes.c_void_p if ptr else _CTYPES[ty]
        fields.append((fname, c * int(n) if n else c))
    return fields


@pytest.mark.parametrize("name,size", [("AwqSampleProc", 16), ("AwqSampleProcArgs", 32)])
def test_ctypes_structs_match_the_header(name, size):
    from autoawq_amd import _lib

    fields = _header_struct(name)
    cls = getattr(_lib, name)
    assert [f for f, _ in fields] == [f for f, _ in cls._fields_]

    class FromHeader(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(cls) == ctypes.sizeof(FromHeader) == size
    for f, _ in fields:
        assert getattr(cls, f).offset == getattr(FromHeader, f).offset, f


def test_new_entry_points_in_the_ctypes_table():
    from autoawq_amd import _lib

    assert {"awq_sample_tokens_ex", "awq_sample_history_seed"} <= set(_lib.SIGNATURES)
