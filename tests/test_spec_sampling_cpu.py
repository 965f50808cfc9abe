"""CPU checks of speculative decoding with the sampler (awq_sample_tokens_slots, awq_spec_accept_ex; generate(draft_accept=
"sampler")): the exported symbols and ctypes mirrors against the header, the entry points' host-side validation, the loop
identity -- a speculative loop whose slots ask "what would the plain sampler emit here" emits the plain sampled run's text exactly
-- and the rate at which a fixed draft is accepted."""
import ctypes

import numpy as np
import pytest

import penalty_ref as pref
import sampling_ref as ref
import spec_ref
import spec_sample_ref as sref
from test_sampling_rows_cpu import _header_struct


def test_symbols_exported_and_structs_match_the_header():
    from autoawq_amd import _lib

    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, cls, arity in (("awq_sample_tokens_slots", _lib.AwqSampleSlotsArgs, 1), ("awq_spec_accept_ex", _lib.AwqSpecArgs, 2)):
        assert hasattr(h, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == arity and args[0] == ctypes.POINTER(cls)
    assert _lib.SIGNATURES["awq_spec_accept_ex"][1][1] == ctypes.POINTER(_lib.AwqSpecHistoryArgs)
    for name, size in (("AwqSampleSlotsArgs", 144), ("AwqSpecHistoryArgs", 32), ("AwqSpecArgs", 144)):
        fields = _header_struct(name)
        cls = getattr(_lib, name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name

        class FromHeader(ctypes.Structure):
            _fields_ = fields

        assert ctypes.sizeof(cls) == ctypes.sizeof(FromHeader) == size, name
        for f, _ in fields:
            assert getattr(cls, f).offset == getattr(FromHeader, f).offset, (name, f)


def _fill(a, B=2, T=4, V=100):
    """arguments that pass every check but were never allocated: each case below breaks one of them, so nothing is launched"""
    a.struct_bytes = ctypes.sizeof(a)
    a.flags = 0
    a.logits, a.B, a.T, a.V, a.row_stride = 0x10000, B, T, V, V
    a.params, a.cnt, a.tok, a.pred = 0x20000, 0x30000, 0x40000, 0x50000
    a.finished, a.status = None, 0x60000
    a.workspace, a.workspace_bytes, a.stream = 0x70000, 1 << 30, None
    a.proc, a.history, a.history_stride = None, None, 0
    return a


CASES = [("T", 1, -3), ("T", 9, -3), ("B", 0, -3), ("V", 0, -3), ("V", (1 << 20) + 1, -3), ("struct_bytes", 8, -1),
         ("struct_bytes", 160, -1), ("row_stride", 99, -1), ("logits", None, -6), ("params", None, -6), ("cnt", None, -6),
         ("tok", None, -6), ("pred", None, -6), ("status", None, -6), ("workspace", None, -6), ("workspace_bytes", 64, -4),
         ("workspace", 0x70010, -2), ("logits", 0x10001, -2), ("params", 0x20004, -2), ("cnt", 0x30002, -2), ("tok", 0x40004, -2),
         ("pred", 0x50004, -2), ("finished", 0x80002, -2)]


@pytest.mark.parametrize("field,value,code", CASES, ids=[f"{f}={v}" for f, v, _ in CASES])
def test_slots_entry_point_refuses_before_any_launch(field, value, code):
    from autoawq_amd import _lib

    a = _fill(_lib.AwqSampleSlotsArgs())
    setattr(a, field, value)
    assert _lib.lib().awq_sample_tokens_slots(ctypes.byref(a)) == code


def test_slots_entry_point_checks_of_its_own():
    from autoawq_amd import _lib

    L = _lib.lib()
    assert L.awq_sample_tokens_slots(None) == -6
    a = _fill(_lib.AwqSampleSlotsArgs(), B=205, T=5)           # B * T = 1025
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -3
    a = _fill(_lib.AwqSampleSlotsArgs(), B=128, T=8)           # 1024 passes the limit: the next broken check answers
    a.workspace_bytes = 64
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -4
    a = _fill(_lib.AwqSampleSlotsArgs())
    a.proc = 0x90000                                           # proc without history
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -6
    a.proc, a.history, a.history_stride = None, 0xA0000, 4     # history without proc
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -6
    a.proc, a.history_stride = 0x90000, 3                      # stride < ceil(V / 32)
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -1
    a.history_stride, a.proc = 4, 0x90008                      # proc 16-byte aligned
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -2
    a.proc, a.history = 0x90000, 0xA0002
    assert L.awq_sample_tokens_slots(ctypes.byref(a)) == -2


def test_accept_ex_refuses_before_any_launch():
    from autoawq_amd import _lib

    L = _lib.lib()
    a = _lib.AwqSpecArgs()
    a.struct_bytes, a.flags, a.B, a.T = ctypes.sizeof(a), 0, 2, 4
    a.params, a.tok, a.pred, a.hist, a.hist_cap, a.n_hist = 0x1000, 0x2000, 0x3000, 0x4000, 16, 0x5000
    a.cnt, a.ring, a.ring_cap, a.finished, a.pos_rows, a.len_rows = 0x6000, 0x7000, 16, 0x8000, 0x9000, 0xA000

    def q(**kw):
        h = _lib.AwqSpecHistoryArgs()
        h.struct_bytes, h.flags, h.history, h.history_stride, h.V = ctypes.sizeof(h), 0, 0xB000, 4, 100
        for k, v in kw.items():
            setattr(h, k, v)
        return ctypes.byref(h)

    assert L.awq_spec_accept_ex(None, q()) == L.awq_spec_accept(None) == -1
    assert L.awq_spec_accept_ex(ctypes.byref(a), q(struct_bytes=24)) == -1
    assert L.awq_spec_accept_ex(ctypes.byref(a), q(flags=1)) == -3
    assert L.awq_spec_accept_ex(ctypes.byref(a), q(V=0)) == -3
    assert L.awq_spec_accept_ex(ctypes.byref(a), q(history=None)) == -6
    assert L.awq_spec_accept_ex(ctypes.byref(a), q(history_stride=3)) == -1
    assert L.awq_spec_accept_ex(ctypes.byref(a), q(history=0xB002)) == -2
    a.T = 9                                                    # the first struct's checks come first, with their codes
    assert L.awq_spec_accept_ex(ctypes.byref(a), q()) == L.awq_spec_accept(ctypes.byref(a)) == -3


def test_generate_refuses_draft_accept_before_any_launch():
    import torch

    from autoawq_amd.modules.fused.decode import GraphedDecoder

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("generate touched the model: " + name)

    dec = GraphedDecoder.__new__(GraphedDecoder)
    dec.batch, dec.device, dec.lm = 3, torch.device("cpu"), Untouchable()
    ids = torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="draft_accept"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, draft_accept="rejection")
    with pytest.raises(ValueError, match="draft_tokens"):
        dec.generate(ids, max_new_tokens=4, draft_accept="sampler")
    with pytest.raises(ValueError, match="per-row"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, draft_accept="sampler", temperature=[1.0, 0.5, 1.0])
    with pytest.raises(ValueError, match="extend"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, draft_accept="sampler", extend=True)
    with pytest.raises(ValueError, match="logprobs"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, draft_accept="sampler", logprobs=True)
    with pytest.raises(ValueError, match="top_p"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, draft_accept="sampler", do_sample=True, top_p=0.0)
    with pytest.raises(ValueError, match="repetition_penalty"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, draft_accept="sampler", repetition_penalty=0.0)


# ---- the loop identity ---------------------------------------------------------------------------------------------------------

V_TOY = 24


def _toy_model(seed):
    """logits [V] fp16 as a function of the last two tokens: peaked, so that the text repeats and prompt lookup finds drafts"""
    table = (np.random.default_rng(seed).standard_normal((V_TOY, V_TOY, V_TOY)) * 1.5).astype(np.float16)
    for a in range(V_TOY):
        table[:, a, (5 * a + 3) % V_TOY] += np.float16(5.0)   # a preferred successor of every token
    return lambda prefix: table[prefix[-2] if len(prefix) > 1 else 0, prefix[-1]]


def _sampler_f(model, prompt, row, eos, *, temperature, seed, repetition_penalty=1.0, min_new_tokens=0):
    """f(prefix) -> the plain sampler's token: t from the prefix length, the ids seen = the whole prefix"""
    def f(prefix):
        t = len(prefix) - len(prompt) + 1
        seen = np.zeros(V_TOY, dtype=bool)
        seen[np.asarray(prefix)] = True
        v = pref.process(model(prefix), seen, t=t, repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, eos_ids=eos)
        return ref.choose(v, do_sample=True, temperature=temperature, seed=seed, t=t, row=row)[0]
    return f


@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("proc", [False, True])
def test_spec_loop_emits_the_plain_sampled_text(T, proc):
    model = _toy_model(3)
    accepted = 0
    for row, (temperature, seed) in enumerate([(0.5, 11), (1.0, 12), (1.3, 2 ** 40 + 7)]):
        prompt = [1, 8, 19, 1, 8][:3 + row]
        kw = dict(repetition_penalty=1.3, min_new_tokens=6) if proc else {}
        free = spec_ref.greedy_loop(_sampler_f(model, prompt, row, (), temperature=temperature, seed=seed, **kw), prompt, 40)
        eos = (free[3],) if proc else ()                      # an id the run emits inside the min_new_tokens window
        f = _sampler_f(model, prompt, row, eos, temperature=temperature, seed=seed, **kw)
        plain = spec_ref.greedy_loop(f, prompt, 40, eos)
        spec, per_step = spec_ref.spec_loop(f, prompt, 40, T, 3, eos)
        assert spec == plain, (row, T)
        assert sum(per_step) + 1 == len(plain)
        if proc:
            assert eos[0] not in plain[:6]                     # suppressed while t <= min_new_tokens
        accepted += sum(n - 1 for n in per_step)
    assert accepted > 0                                        # some drafts were accepted: the identity was exercised past slot 0


def test_a_fixed_draft_is_accepted_at_the_rejection_sampling_rate():
    """exact-match acceptance of a point-mass draft d: P(accept) = P(the sampler draws d) = p(d), min(1, p / q) with q = 1.  Over
    2000 seeds the share of draws equal to d lies within 4 binomial standard deviations of p(d)."""
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal(16) * 2.0).astype(np.float16)
    n = 2000
    for cfg in (dict(temperature=1.0), dict(temperature=0.7, top_k=8, top_p=0.9)):
        p = ref.probabilities(logits, **cfg)
        draft = int(np.argsort(p)[-2])                         # the runner-up: neither rare nor certain
        hits = sum(ref.choose(logits, do_sample=True, seed=s, t=3, row=1, **cfg)[0] == draft for s in range(n))
        sd = np.sqrt(p[draft] * (1 - p[draft]) / n)
        print(f"{cfg}: p(draft) {p[draft]:.4f}, accepted {hits / n:.4f}, sd {sd:.4f}")
        assert abs(hits / n - p[draft]) <= 4 * sd
