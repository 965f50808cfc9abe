"""Token log-probabilities without a GPU: the C ABI's symbol and its host-side refusals (no launch), the error bound of
tests/logprob_bound.py against a float32 restatement of the kernel's order of operations, and the argument checks of
GraphedDecoder.generate(logprobs=True) that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import logprob_bound as lb
from conftest import ROOT


def _lib():
    from autoawq_amd import _lib

    if not _lib.available():
        import __graft_entry__

        __graft_entry__.build()
    return _lib


def test_symbol_in_header_library_and_ctypes_table():
    _l = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "awq_hip.h")).read(), flags=re.S)
    assert re.search(r"AWQ_EXPORT int awq_token_logprobs\(const AwqLogprobArgs\* args\);", src)
    fields = re.search(r"typedef struct AwqLogprobArgs \{(.*?)\} AwqLogprobArgs;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == [n for n, _ in _l.AwqLogprobArgs._fields_]      # same fields, same order
    assert ctypes.sizeof(_l.AwqLogprobArgs) == 11 * 8
    assert "awq_token_logprobs" in _l.SIGNATURES
    assert hasattr(ctypes.CDLL(_l.LIB_PATH), "awq_token_logprobs")


def _args(_l, **kw):
    a = _l.AwqLogprobArgs()
    a.logits, a.ids, a.out = 0x10000, 0x20000, 0x30000   # never dereferenced: every call below returns before a launch
    a.logits_stride, a.ids_stride, a.out_stride, a.R, a.V = 32000, 1, 1, 4, 32000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_host_side_refusals_return_their_code_without_a_launch():
    _l = _lib()
    f = _l.lib().awq_token_logprobs
    NULL, BAD_SHAPE = -6, -1
    assert f(None) == NULL
    for kw in ({"V": 0}, {"V": -5}, {"V": (1 << 20) + 1}, {"R": -1}, {"R": 1 << 31}, {"logits_stride": 31999},
               {"R": 1, "logits_stride": 31999}, {"R": 0, "V": 0}):
        assert f(ctypes.byref(_args(_l, **kw))) == BAD_SHAPE, kw
    for kw in ({"logits": None}, {"ids": None}, {"out": None}):
        assert f(ctypes.byref(_args(_l, **kw))) == NULL, kw
    assert f(ctypes.byref(_args(_l, R=0))) == 0                                        # nothing to do: OK, no launch
    assert f(ctypes.byref(_args(_l, R=0, logits=None, ids=None, out=None))) == 0
    assert f(ctypes.byref(_args(_l, V=1 << 20, logits_stride=1 << 20, R=0))) == 0      # the largest vocabulary is legal
    assert _l.lib().awq_hip_error_string(BAD_SHAPE).decode().startswith("bad shape")


def test_ops_refuse_cpu_tensors_dtypes_and_shapes():
    from autoawq_amd import ops
    from autoawq_amd._lib import AwqHipError

    lg, ids = torch.zeros((2, 16), dtype=torch.float16), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(AwqHipError, match="HIP device"):
        ops.token_logprobs(lg, ids)
    with pytest.raises(AwqHipError, match="HIP device"):
        ops.token_logprobs_launch(lg, ids, torch.zeros(2))
    for bad_lg, bad_ids, msg in ((lg.float(), ids, "fp16 logits"), (lg, ids.int(), "ids must be int64"),
                                 (lg, torch.zeros(3, dtype=torch.int64), "ids must be int64"),
                                 (torch.zeros((2, 3, 16), dtype=torch.float16), ids, "ids must be int64"),
                                 (lg[:, ::2], ids, "contiguous")):
        with pytest.raises(AwqHipError, match=msg):
            ops.token_logprobs(bad_lg, bad_ids)
    with pytest.raises(AwqHipError, match="out must be"):
        ops.token_logprobs(lg, ids, out=torch.zeros(2, dtype=torch.float16))


def test_header_formulas_are_the_ones_the_bound_uses():
    """csrc/logprob.hip states its summation depth and exp count as formulas of V; tests/logprob_bound.py restates them."""
    src = open(os.path.join(ROOT, "autoawq_amd", "csrc", "logprob.hip")).read()
    assert "= 9 steps + 20." in src and "= steps + 11." in src and "kThreads = 1024" in src and "kVec = 8" in src
    assert lb.depths(1) == (29, 12) and lb.depths(8192) == (29, 12) and lb.depths(8193) == (38, 13)
    assert lb.depths(32000) == (9 * 4 + 20, 4 + 11) and lb.depths(128256) == (9 * 16 + 20, 16 + 11)


VOCABS = (1, 7, 2049, 8193, 32000, 128256)


@pytest.mark.parametrize("V", VOCABS)
def test_bound_holds_for_a_float32_restatement_of_the_kernel(V):
    """Both load paths' orders, the seven row kinds, targets 0, V // 2, V - 1 and the argmax: the restatement (whose exp is
    correctly rounded where the hardware's is within an ulp) stays well inside the bound -- and the bound is not vacuous."""
    rng = np.random.default_rng(V)
    worst = 0.0
    for kind in lb.KINDS:
        row = lb.make_row(kind, V, rng)
        for i in lb.targets(row):
            want, bound = lb.logprob_bound(row, [i])
            if kind == "flat":
                assert abs(want[0] + np.log(V)) <= 1e-12 * max(1.0, np.log(V))
            for vec in (True, False):
                got = lb.emulate(row, i, vec)
                ok, ratio = lb.check([got], want, bound)
                assert ok.all(), (kind, i, vec, float(got), want[0], ratio[0])
                worst = max(worst, float(ratio[0]))
            if np.isfinite(want[0]):
                assert 0 < bound[0] < 1e-3 * max(1.0, abs(want[0])), (kind, i, bound[0])
    print(f"V = {V}: worst error / bound of the restatement {worst:.3f}")


def test_contract_cases_of_the_reference():
    inf = np.inf
    x = np.array([[0.0, 1.0, -inf, 2.0], [-inf, 3.0, -inf, -inf], [-inf] * 4, [0.0, np.nan, 0.0, 0.0], [0.0, inf, 0.0, 0.0],
                  [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]], np.float16)
    want, bound = lb.logprob_bound(x, [2, 1, 0, 0, 0, -1, 4])
    assert want[0] == -inf and want[1] == 0.0 and np.isnan(want[2]) and np.isnan(want[3]) and np.isnan(want[4])
    assert want[5] == 0.0 and bound[5] == 0.0 and np.isnan(want[6])
    ok, _ = lb.check([-inf, 0.0, np.nan, np.nan, np.nan, 0.0, np.nan], want, bound)
    assert ok.all()
    ok, _ = lb.check([-1e30, 0.0, 0.0, np.nan, -3.0, np.nan, 0.0], want, bound)   # NaN only where the contract says so, and required there
    assert ok.tolist() == [False, True, False, True, False, False, False]
    assert lb.emulate(x[1], 1) == 0.0 and lb.emulate(x[0], 2) == -inf and np.isnan(lb.emulate(x[2], 0))


@pytest.mark.parametrize("V", (2049, 32000))
def test_bound_is_sensitive_dropping_a_heavy_logit_moves_the_reference_by_100_bounds(V):
    """A logit that carries >= 10 % of the row's mass: the reference without it lies > 100 bounds away, wherever it sits."""
    rng = np.random.default_rng(7 + V)
    row = (rng.standard_normal(V) * 1.5).astype(np.float16)
    top = float(row.astype(np.float32).max())
    for at in (0, 7, 8, V // 2, V - 1):
        x = row.copy()
        x[x.astype(np.float32) >= top] = np.float16(top - 2.0)
        x[at] = np.float16(top + np.log(V) / 2)        # heavy: a good share of the mass of V logits of spread 1.5
        i = (at + 1) % V
        want, bound = lb.logprob_bound(x, [i])
        p = np.exp(x.astype(np.float64) - float(x[at]))
        assert p[at] / p.sum() >= 0.10, p[at] / p.sum()
        without, _ = lb.logprob_bound(x, [i], drop=[at])
        margin = lb.needle_margin(want, without, bound)[0]
        assert margin > 100, (at, margin)


def test_owner_map_matches_the_two_load_paths():
    assert lb.owner(0) == (0, 0, 0) and lb.owner(7) == (0, 0, 7) and lb.owner(8) == (0, 1, 0) and lb.owner(8191) == (0, 1023, 7)
    assert lb.owner(8192) == (1, 0, 0) and lb.owner(512) == (0, 64, 0)
    assert lb.owner(0, False) == (0, 0, 0) and lb.owner(1, False) == (0, 1, 0) and lb.owner(1024, False) == (0, 0, 1)
    assert lb.owner(8191, False) == (0, 1023, 7) and lb.owner(8192 + 1025, False) == (1, 1, 1)


def test_generate_refuses_logprobs_with_draft_tokens_before_any_launch():
    """draft_tokens with logprobs raises ValueError from the argument checks, scalar and per-row, before generate touches the
    model (a decoder whose model raises on any use); the other refusals stay what they were with logprobs on."""
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("generate touched the model: " + name)

    dec = GraphedDecoder.__new__(GraphedDecoder)
    dec.batch, dec.device, dec.lm = 3, torch.device("cpu"), Untouchable()
    dec.last_logprobs = "stale"
    ids = torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="logprobs"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, logprobs=True)
    with pytest.raises(ValueError, match="logprobs"):
        dec.generate(ids, max_new_tokens=[4, 4, 4], draft_tokens=3, logprobs=True)
    with pytest.raises(ValueError, match="draft_tokens"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, extend=True)            # as before
    with pytest.raises(ValueError, match="max_new_tokens"):
        dec.generate(ids, max_new_tokens=0, logprobs=True)
    assert dec.last_logprobs is None                                                # reset before the argument checks
    with pytest.raises(ValueError, match="row 1"):
        dec.generate(ids, max_new_tokens=[4, 0, 4], logprobs=True)
    with pytest.raises(ValueError):
        dec.generate(ids[:2], max_new_tokens=4, logprobs=True)
    with pytest.raises(ValueError):
        dec.score(ids[:2])
    with pytest.raises(ValueError):
        dec.score(ids[:, :0])
