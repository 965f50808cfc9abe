"""QuantAttentionFused.forward_qkv, characterised on the CPU: which `ops` functions every kind of call runs, in which order and
with which arguments.  `ops`, `F.scaled_dot_product_attention` and `_attend_torch` are replaced by a recorder that logs each call
(scalars by value, tensors by a tag saying WHICH tensor it is, plus shape and dtype; arguments left at the function's default are
not listed) and returns zeros of the documented shape.  EXPECTED below was printed by `python tests/test_attn_step_cpu.py` on the
commit BEFORE the step description (AttnStep) existed and is committed unchanged: the same table holds before and after.  On that
commit `_configure` and `_call` fall back to the attributes of the time (`decode_len_bound`, `verify_rows`, `extend_rows`, set and
restored around the call as LlamaLikeModel.forward did), the three-line adapters below.

One argument is recorded as "ignored" on both sides: `max_len` of a decode launch that has no device length word.  The launcher
sizes the split from the host length there (csrc/decoder.hip, awq_launch_decode_attention:
`len_for_split = a.len_dev ? max_len : seq_len + (fused ? 1 : 0)`), so the value never reaches a kernel."""
import inspect
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from autoawq_amd import ops as real_ops
from autoawq_amd.modules.fused import attn as attn_mod
from autoawq_amd.modules.fused.attn import QuantAttentionFused

B, TMAX = 2, 16
DTYPE = {torch.float16: "f16", torch.float32: "f32", torch.int32: "i32", torch.uint8: "u8"}
OPS = ("rope_kv_append", "decode_attention_rope", "decode_attention", "prefill_attention", "prefill_attention_rows",
       "verify_attention_rows", "kv_dequant_fp8")


class Recorder:
    def __init__(self):
        self.log, self.tags, self.module = [], [], None  # tags: (storage pointer, name, tensor kept alive)
        for name in OPS:
            setattr(self, name, self._op(name))

    def tag(self, t, name):
        self.tags.append((t.untyped_storage().data_ptr(), name, t))
        return t

    def _describe(self, v):
        if not isinstance(v, torch.Tensor):
            return v if v == "ignored" else repr(v)
        m, ptr, name = self.module, v.untyped_storage().data_ptr(), "tensor"
        named = {"cache.k": m.cache.k, "cache.v": m.cache.v, "k_scale": m.cache.k_scale, "v_scale": m.cache.v_scale,
                 "cos": m.rope.cos, "sin": m.rope.sin, "alibi.slopes": m.alibi.slopes if m.alibi is not None else None}
        for n, t in named.items():  # k / v (and their scales) are two halves of one allocation: the offset tells them apart
            if t is not None and t.untyped_storage().data_ptr() == ptr and \
                    t.storage_offset() <= v.storage_offset() < t.storage_offset() + t.numel():
                name = n if v.shape == t.shape else n + " view"
        for p, n, _ in self.tags:
            if p == ptr:
                name = n
        return f"{name}{list(v.shape)}:{DTYPE[v.dtype]}".replace(" ", "")

    def _record(self, name, args, out):
        self.log.append(f"{name}({', '.join(f'{k}={self._describe(v)}' for k, v in args.items())})")
        return self.tag(out, name + ".out")

    def _op(self, name):
        sig = inspect.signature(getattr(real_ops, name))

        def call(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            full = bound.arguments
            args = {k: v for k, v in full.items() if isinstance(v, torch.Tensor) or v != sig.parameters[k].default}
            # a decode launch without a device length word never reads max_len (see the module docstring)
            if name.startswith("decode_attention") and all(full.get(w) is None for w in ("len_dev", "len_rows", "pos_dev", "pos_rows")):
                args = {k: "ignored" if k == "max_len" else args[k] for k in full if k in args or k == "max_len"}
            if name == "kv_dequant_fp8":
                c = full["cache"]
                out = torch.zeros((full["batch"], full["n"], c.shape[2], c.shape[3]), dtype=torch.float16)
            elif name == "rope_kv_append":
                out = torch.zeros(tuple(full["qkv"].shape[:2]) + (full["n_heads"], full["head_dim"]), dtype=torch.float16)
            elif name == "decode_attention_rope":
                out = torch.zeros((full["qkv"].shape[0], full["n_heads"], full["k_cache"].shape[3]), dtype=torch.float16)
            else:
                out = torch.zeros_like(full["q"])
            return self._record(name, args, out)
        return call

    def sdpa(self, q, k, v, attn_mask=None, is_causal=False):
        args = {"q": q, "k": k, "v": v}
        if attn_mask is not None:  # the mask by content: how many cache rows each query sees
            args["attn_mask_row_sums"] = tuple(attn_mask.sum(dim=-1).tolist())
        if is_causal:
            args["is_causal"] = True
        return self._record("sdpa", args, torch.zeros_like(q))

    def attend_torch(self, q, k, v, first_q_pos):
        return self._record("_attend_torch", {"q": q, "k": k, "v": v, "first_q_pos": first_q_pos}, torch.zeros_like(q))


class Proj(nn.Module):
    """stand-in for o_proj: zeros [B, S, hidden], tagged"""

    def __init__(self, rec, width):
        super().__init__()
        self.rec, self.width = rec, width

    def forward(self, x):
        return self.rec.tag(torch.zeros(x.shape[:-1] + (self.width,), dtype=torch.float16), "o_proj.out")


class HeadNorm(nn.Module):
    def forward(self, x):
        return x * 1.0


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(attn_mod, "ops", r)
    monkeypatch.setattr(attn_mod, "F", SimpleNamespace(scaled_dot_product_attention=r.sdpa))
    return r


def _module(rec, heads=(2, 1, 128), **kw):
    hq, hkv, d = heads
    m = QuantAttentionFused(hq * d, hq, hkv, None, Proj(rec, hq * d), "cpu", max_seq_len=TMAX, head_dim=d, **kw)
    m._attend_torch = rec.attend_torch
    rec.module = m
    return m


def _words(rec):
    w = {n: rec.tag(torch.zeros(1 if n in ("pos", "len") else B, dtype=torch.int32), n)
         for n in ("pos", "len", "pos_rows", "len_rows", "count_rows")}
    return SimpleNamespace(**w)


def _configure(m, pos, ln, per_row=False, bound=None):
    if "bound" in inspect.signature(m.use_device_positions).parameters:
        return m.use_device_positions(pos, ln, per_row=per_row, bound=bound)
    m.use_device_positions(pos, ln, per_row=per_row)  # the commit before: the bound was a bare attribute
    m.decode_len_bound = bound


def _forward_qkv(m, xqkv, apply_o_proj, request):
    if "request" in inspect.signature(m.forward_qkv).parameters:
        return m.forward_qkv(xqkv, apply_o_proj, request=request)
    m.verify_rows, m.extend_rows = request == "verify", None if request in (None, "verify") else tuple(request)
    try:  # the commit before: LlamaLikeModel.forward set and restored these around the call
        return m.forward_qkv(xqkv, apply_o_proj)
    finally:
        m.verify_rows, m.extend_rows = False, None


def _call(rec, m, seqlen, request=None, apply_o_proj=True, want_start=None):
    """one forward_qkv call -> its log lines, after asserting the returned triple, start_pos and the past_key_value stub"""
    rec.log = []
    hq, hkv, d = m.n_heads, m.n_kv_heads, m.head_dim
    xqkv = rec.tag(torch.zeros((B, seqlen, (hq + 2 * hkv) * d), dtype=torch.float16), "xqkv")
    before = m.start_pos if m.cache_batch_size == B else 0  # (the first call resizes the cache from batch 1 and starts at 0)
    out, heads, past = _forward_qkv(m, xqkv, apply_o_proj, request)
    assert heads.shape == (B, seqlen, hq * d) and heads.dtype == torch.float16
    assert rec._describe(out).startswith("o_proj.out") if apply_o_proj else out is heads
    assert m.start_pos == (before if request is not None else before + seqlen)
    if want_start is not None:
        assert m.start_pos == want_start
    assert len(past) == 1 and past[0].shape == (1, 1, m.start_pos, 1)
    return rec.log + [f"-> start_pos {m.start_pos}"]


def _sequence(rec, m, rows=True):
    """prefill 3 at 0, chunked prefill 2 at 3, then a decode step with every position source in turn"""
    w = _words(rec)
    log = {"prefill 3 @0": _call(rec, m, 3, want_start=3), "prefill 2 @3": _call(rec, m, 2, want_start=5),
           "decode host": _call(rec, m, 1, want_start=6)}
    _configure(m, w.pos, w.len, bound=8)
    log["decode shared bound 8"] = _call(rec, m, 1, apply_o_proj=False)
    log["prefill 2 with device words set"] = _call(rec, m, 2)
    _configure(m, w.pos, w.len)
    log["decode shared"] = _call(rec, m, 1)
    if rows:
        _configure(m, w.pos_rows, w.len_rows, per_row=True, bound=99)  # (clamped to the window)
        log["decode rows bound 99"] = _call(rec, m, 1)
    _configure(m, None, None)
    log["decode host again"] = _call(rec, m, 1, want_start=12 if rows else 11)
    return log


CONFIGS = {
    "fp16": {}, "fp16 softcap": {"attn_logit_softcapping": 30.0}, "fp16 alibi": {"use_alibi": True},
    "fp8": {"kv_cache_dtype": "fp8"}, "fp8 softcap": {"kv_cache_dtype": "fp8", "attn_logit_softcapping": 30.0},
    "fp8 alibi": {"kv_cache_dtype": "fp8", "use_alibi": True},
    "partial rotary": {"partial_rotary_factor": 0.5},
    "q_norm k_norm": {"q_norm": HeadNorm(), "k_norm": HeadNorm()},
}
SWITCHES = {"no fused rope": {"FUSE_ROPE_INTO_ATTENTION": False}, "no prefill kernel": {"PREFILL_KERNEL": False},
            "fp8 no prefill kernel": {"PREFILL_KERNEL": False}}
NON_NATIVE = {"3/1x128": ((3, 1, 128), {}), "3/1x128 softcap": ((3, 1, 128), {"attn_logit_softcapping": 30.0}),
              "2/2x64": ((2, 2, 64), {}), "2/2x64 alibi": ((2, 2, 64), {"use_alibi": True})}


def _requests(rec):
    """verify and extend steps; the host's start_pos (5 after the prefill) must not move"""
    log = {}
    for name, kw in (("fp16", {}), ("fp16 alibi", {"use_alibi": True}), ("fp8", {"kv_cache_dtype": "fp8"})):
        m, w = _module(rec, **kw), _words(rec)
        _call(rec, m, 3), _call(rec, m, 2)
        ext = (w.pos_rows, w.count_rows)
        log[f"extend {name} S 3 max_end 9"] = _call(rec, m, 3, request=ext + (9,), want_start=5)
        log[f"extend {name} max_end 0"] = _call(rec, m, 1, request=ext + (0,), apply_o_proj=False, want_start=5)
        log[f"extend {name} max_end 16"] = _call(rec, m, 2, request=ext + (TMAX,), want_start=5)
    m, w = _module(rec), _words(rec)
    _call(rec, m, 3), _call(rec, m, 2)
    _configure(m, w.pos_rows, w.len_rows, per_row=True)
    log["verify T 2"] = _call(rec, m, 2, request="verify", want_start=5)
    log["verify T 8"] = _call(rec, m, 8, request="verify", apply_o_proj=False, want_start=5)
    _configure(m, w.pos_rows, w.len_rows, per_row=True, bound=4)
    log["verify T 2 bound 4"] = _call(rec, m, 2, request="verify", want_start=5)
    log["verify T 8 bound 4"] = _call(rec, m, 8, request="verify", want_start=5)
    log["decode rows after verify"] = _call(rec, m, 1, want_start=6)
    return log


def record_all(rec):
    table = {}
    for name, kw in CONFIGS.items():
        table[name] = _sequence(rec, _module(rec, **kw))
    for name, switch in SWITCHES.items():
        m = _module(rec, **({"kv_cache_dtype": "fp8"} if name.startswith("fp8") else {}))
        for k, v in switch.items():
            setattr(m, k, v)  # (on the instance: the class default stays)
        table[name] = _sequence(rec, m)
    for name, (heads, kw) in NON_NATIVE.items():
        table[name] = _sequence(rec, _module(rec, heads=heads, **kw), rows=False)
    table["requests"] = _requests(rec)
    return table


def _flat(table):
    return [f"{case} | {call} | {line}" for case, calls in table.items() for call, lines in calls.items() for line in lines]


def test_every_call_runs_the_recorded_launches(rec):
    got, want = _flat(record_all(rec)), _flat(EXPECTED)
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_forward_projects_then_runs_forward_qkv(rec):
    m = _module(rec)
    m.qkv_proj = lambda h: rec.tag(torch.zeros((B, 3, 4 * 128), dtype=torch.float32), "xqkv")  # (forward casts to fp16)
    out, heads, past = m.forward(torch.zeros((B, 3, 256), dtype=torch.float16))
    assert [line.split("(")[0] for line in rec.log] == ["rope_kv_append", "prefill_attention"]
    assert out.shape == heads.shape == (B, 3, 256) and m.start_pos == 3 and past[0].shape == (1, 1, 3, 1)


def _refused(rec, m, seqlen, request, exc, message):
    """the call raises, launches what the table says it launches before it does, and leaves start_pos alone"""
    start, rec.log = m.start_pos, []
    xqkv = rec.tag(torch.zeros((B, seqlen, (m.n_heads + 2 * m.n_kv_heads) * m.head_dim), dtype=torch.float16), "xqkv")
    with pytest.raises(exc) as e:
        _forward_qkv(m, xqkv, True, request)
    assert str(e.value) == message and m.start_pos == start
    return [line.split("(")[0] for line in rec.log]


VERIFY_SHAPE = ("a verify step takes 2 .. 8 tokens, head_dim 128, 1, 2, 4 or 8 query heads per KV head, no ALiBi and no soft cap")
VERIFY_ROWS = "a verify step needs per-row device positions (use_device_positions(..., per_row=True))"
VERIFY_FP8 = 'speculative decoding: kv_cache_dtype="fp8" is not supported (verify_attention_rows reads fp16 caches)'
EXTEND_SHAPE = "an extend step takes head_dim 128 and 1, 2, 4 or 8 query heads per KV head"
ROWS_SHAPE = "per-row decode positions need the native decode attention (head_dim 128, 1, 2, 4 or 8 query heads per KV head)"


def test_refusals_and_the_plain_call_after_them(rec):
    """type, message and order of every refusal; no refusal launches anything except the per-row decode on a non-native shape,
    which appends first (as before); and the next plain call on the same module is a plain call"""
    w = _words(rec)
    m = _module(rec)
    _call(rec, m, 3)
    assert _refused(rec, m, 2, "verify", RuntimeError, VERIFY_ROWS) == []                  # no per-row words
    _configure(m, w.pos, w.len)
    assert _refused(rec, m, 2, "verify", RuntimeError, VERIFY_ROWS) == []                  # shared words are not per-row words
    _configure(m, w.pos_rows, w.len_rows, per_row=True)
    for T in (1, 9):
        assert _refused(rec, m, T, "verify", NotImplementedError, VERIFY_SHAPE) == []
    ext = (w.pos_rows, w.count_rows)
    for end in (-1, TMAX + 1):
        assert _refused(rec, m, 2, ext + (end,), ValueError, f"extend: max_end {end} outside the cache window {TMAX}") == []
    assert [l.split("(")[0] for l in _call(rec, m, 2, want_start=5)[:-1]] == ["rope_kv_append", "prefill_attention"]
    assert [l.split("(")[0] for l in _call(rec, m, 1, want_start=6)[:-1]] == ["decode_attention_rope"]
    assert "pos_rows=pos_rows" in rec.log[0]

    m = _module(rec, kv_cache_dtype="fp8")  # fp8 is refused before the missing per-row words are
    assert _refused(rec, m, 2, "verify", NotImplementedError, VERIFY_FP8) == []
    for kw in ({"use_alibi": True}, {"attn_logit_softcapping": 30.0}):
        m = _module(rec, **kw)
        _configure(m, w.pos_rows, w.len_rows, per_row=True)
        assert _refused(rec, m, 2, "verify", NotImplementedError, VERIFY_SHAPE) == []

    m = _module(rec, heads=(3, 1, 128))
    _call(rec, m, 3)
    assert _refused(rec, m, 2, "verify", RuntimeError, VERIFY_ROWS) == []                  # the words are asked for before the shape
    assert _refused(rec, m, 2, ext + (99,), NotImplementedError, EXTEND_SHAPE) == []       # the shape before the window
    _configure(m, w.pos_rows, w.len_rows, per_row=True)
    assert _refused(rec, m, 2, "verify", NotImplementedError, VERIFY_SHAPE) == []
    assert _refused(rec, m, 1, None, NotImplementedError, ROWS_SHAPE) == ["rope_kv_append"]
    assert [l.split("(")[0] for l in _call(rec, m, 2, want_start=5)[:-1]] == ["rope_kv_append", "prefill_attention"]
    _configure(m, None, None)
    assert [l.split("(")[0] for l in _call(rec, m, 1, want_start=6)[:-1]] == ["rope_kv_append", "sdpa"]

    with pytest.raises(ValueError, match="kv_cache_dtype='fp8' needs head_dim 128 and 1, 2, 4 or 8 query heads per KV head"):
        _module(rec, heads=(3, 1, 128), kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="per_row needs both the position and the length words"):
        m.use_device_positions(w.pos_rows, None, per_row=True)


EXPECTED = {
 'fp16': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, max_len=ignored)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=8)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=16)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, max_len=16, pos_rows=pos_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, max_len=ignored)',
   '-> start_pos 12',
  ],
 },
 'fp16 softcap': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0, softcap=30.0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3, softcap=30.0)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=6, max_len=ignored, softcap=30.0)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=7, len_dev=len[1]:i32, max_len=8, softcap=30.0)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7, softcap=30.0)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=10, len_dev=len[1]:i32, max_len=16, softcap=30.0)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=11, max_len=16, softcap=30.0, len_rows=len_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=12, max_len=ignored, softcap=30.0)',
   '-> start_pos 12',
  ],
 },
 'fp16 alibi': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=5, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=6, max_len=ignored, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=6, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=7, len_dev=len[1]:i32, max_len=8, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=9, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=10, len_dev=len[1]:i32, max_len=16, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=10, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_rows=pos_rows[2]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=11, max_len=16, alibi_slopes=alibi.slopes[2]:f32, len_rows=len_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=11, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=12, max_len=ignored, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 12',
  ],
 },
 'fp8': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=3, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=3, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=kv_dequant_fp8.out[2,3,1,128]:f16, v_cache=kv_dequant_fp8.out[2,3,1,128]:f16, start_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=5, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=5, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,5,1,128]:f16, v_cache=kv_dequant_fp8.out[2,5,1,128]:f16, start_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, max_len=ignored, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=8, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=9, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=9, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,9,1,128]:f16, v_cache=kv_dequant_fp8.out[2,9,1,128]:f16, start_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=16, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, max_len=16, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, max_len=ignored, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 12',
  ],
 },
 'fp8 softcap': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=3, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=3, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=kv_dequant_fp8.out[2,3,1,128]:f16, v_cache=kv_dequant_fp8.out[2,3,1,128]:f16, start_pos=0, softcap=30.0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=5, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=5, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,5,1,128]:f16, v_cache=kv_dequant_fp8.out[2,5,1,128]:f16, start_pos=3, softcap=30.0)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=6, max_len=ignored, softcap=30.0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=7, len_dev=len[1]:i32, max_len=8, softcap=30.0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=9, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=9, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,9,1,128]:f16, v_cache=kv_dequant_fp8.out[2,9,1,128]:f16, start_pos=7, softcap=30.0)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=10, len_dev=len[1]:i32, max_len=16, softcap=30.0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=11, max_len=16, softcap=30.0, len_rows=len_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=12, max_len=ignored, softcap=30.0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 12',
  ],
 },
 'fp8 alibi': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=3, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=3, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=kv_dequant_fp8.out[2,3,1,128]:f16, v_cache=kv_dequant_fp8.out[2,3,1,128]:f16, start_pos=0, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=5, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=5, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,5,1,128]:f16, v_cache=kv_dequant_fp8.out[2,5,1,128]:f16, start_pos=3, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=5, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=6, max_len=ignored, alibi_slopes=alibi.slopes[2]:f32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=6, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_dev=pos[1]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=7, len_dev=len[1]:i32, max_len=8, alibi_slopes=alibi.slopes[2]:f32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=9, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=9, batch=2)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,9,1,128]:f16, v_cache=kv_dequant_fp8.out[2,9,1,128]:f16, start_pos=7, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=9, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_dev=pos[1]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=10, len_dev=len[1]:i32, max_len=16, alibi_slopes=alibi.slopes[2]:f32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=10, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=11, max_len=16, alibi_slopes=alibi.slopes[2]:f32, len_rows=len_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=11, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, seq_len=12, max_len=ignored, alibi_slopes=alibi.slopes[2]:f32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 12',
  ],
 },
 'partial rotary': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=5, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=6, max_len=ignored)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=6, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=7, len_dev=len[1]:i32, max_len=8)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=9, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=10, len_dev=len[1]:i32, max_len=16)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=10, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64, pos_rows=pos_rows[2]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=11, max_len=16, len_rows=len_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=11, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=64)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=12, max_len=ignored)',
   '-> start_pos 12',
  ],
 },
 'q_norm k_norm': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=tensor[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=tensor[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'decode_attention_rope(qkv=tensor[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, max_len=ignored)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'decode_attention_rope(qkv=tensor[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=8)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=tensor[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'decode_attention_rope(qkv=tensor[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=16)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'decode_attention_rope(qkv=tensor[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, max_len=16, pos_rows=pos_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'decode_attention_rope(qkv=tensor[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, max_len=ignored)',
   '-> start_pos 12',
  ],
 },
 'no fused rope': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=6, max_len=ignored)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=7, len_dev=len[1]:i32, max_len=8)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=10, len_dev=len[1]:i32, max_len=16)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=11, max_len=16, len_rows=len_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'decode_attention(q=rope_kv_append.out[2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, seq_len=12, max_len=ignored)',
   '-> start_pos 12',
  ],
 },
 'no prefill kernel': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'sdpa(q=rope_kv_append.out[2,2,3,128]:f16, k=tensor[2,2,3,128]:f16, v=tensor[2,2,3,128]:f16, is_causal=True)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'sdpa(q=rope_kv_append.out[2,2,2,128]:f16, k=tensor[2,2,5,128]:f16, v=tensor[2,2,5,128]:f16, attn_mask_row_sums=(4, 5))',
   '-> start_pos 5',
  ],
  'decode host': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, max_len=ignored)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=8)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'sdpa(q=rope_kv_append.out[2,2,2,128]:f16, k=tensor[2,2,9,128]:f16, v=tensor[2,2,9,128]:f16, attn_mask_row_sums=(8, 9))',
   '-> start_pos 9',
  ],
  'decode shared': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=16)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, max_len=16, pos_rows=pos_rows[2]:i32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, max_len=ignored)',
   '-> start_pos 12',
  ],
 },
 'fp8 no prefill kernel': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=3, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=3, batch=2)',
   'sdpa(q=rope_kv_append.out[2,2,3,128]:f16, k=tensor[2,2,3,128]:f16, v=tensor[2,2,3,128]:f16, is_causal=True)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=5, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=5, batch=2)',
   'sdpa(q=rope_kv_append.out[2,2,2,128]:f16, k=tensor[2,2,5,128]:f16, v=tensor[2,2,5,128]:f16, attn_mask_row_sums=(4, 5))',
   '-> start_pos 5',
  ],
  'decode host': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, max_len=ignored, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=8, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=9, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=9, batch=2)',
   'sdpa(q=rope_kv_append.out[2,2,2,128]:f16, k=tensor[2,2,9,128]:f16, v=tensor[2,2,9,128]:f16, attn_mask_row_sums=(8, 9))',
   '-> start_pos 9',
  ],
  'decode shared': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=2, n_kv_heads=1, pos_dev=pos[1]:i32, max_len=16, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 10',
  ],
  'decode rows bound 99': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=2, n_kv_heads=1, max_len=16, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 11',
  ],
  'decode host again': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=11, n_heads=2, n_kv_heads=1, max_len=ignored, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32)',
   '-> start_pos 12',
  ],
 },
 '3/1x128': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,3,3,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,3,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'sdpa(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,6,128]:f16, v=tensor[2,3,6,128]:f16)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   'sdpa(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,7,128]:f16, v=tensor[2,3,7,128]:f16)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,3,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   'sdpa(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,10,128]:f16, v=tensor[2,3,10,128]:f16)',
   '-> start_pos 10',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'sdpa(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,11,128]:f16, v=tensor[2,3,11,128]:f16)',
   '-> start_pos 11',
  ],
 },
 '3/1x128 softcap': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,3,3,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=0, softcap=30.0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=3, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,3,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=3, softcap=30.0)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   '_attend_torch(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,6,128]:f16, v=tensor[2,3,6,128]:f16, first_q_pos=5)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=6, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   '_attend_torch(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,7,128]:f16, v=tensor[2,3,7,128]:f16, first_q_pos=6)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=7, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   'prefill_attention(q=rope_kv_append.out[2,2,3,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, start_pos=7, softcap=30.0)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=9, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_dev=pos[1]:i32)',
   '_attend_torch(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,10,128]:f16, v=tensor[2,3,10,128]:f16, first_q_pos=9)',
   '-> start_pos 10',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,640]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=10, n_heads=3, n_kv_heads=1, head_dim=128, rotary_dim=128)',
   '_attend_torch(q=rope_kv_append.out[2,3,1,128]:f16, k=tensor[2,3,11,128]:f16, v=tensor[2,3,11,128]:f16, first_q_pos=10)',
   '-> start_pos 11',
  ],
 },
 '2/2x64': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=0, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64)',
   'sdpa(q=rope_kv_append.out[2,2,3,64]:f16, k=cache.kview[2,2,3,64]:f16, v=cache.vview[2,2,3,64]:f16, is_causal=True)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=3, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64)',
   'sdpa(q=rope_kv_append.out[2,2,2,64]:f16, k=cache.kview[2,2,5,64]:f16, v=cache.vview[2,2,5,64]:f16, attn_mask_row_sums=(4, 5))',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=5, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64)',
   'sdpa(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,6,64]:f16, v=cache.vview[2,2,6,64]:f16)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=6, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64, pos_dev=pos[1]:i32)',
   'sdpa(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,7,64]:f16, v=cache.vview[2,2,7,64]:f16)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=7, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64)',
   'sdpa(q=rope_kv_append.out[2,2,2,64]:f16, k=cache.kview[2,2,9,64]:f16, v=cache.vview[2,2,9,64]:f16, attn_mask_row_sums=(8, 9))',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=9, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64, pos_dev=pos[1]:i32)',
   'sdpa(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,10,64]:f16, v=cache.vview[2,2,10,64]:f16)',
   '-> start_pos 10',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[16,32]:f32, sin=sin[16,32]:f32, start_pos=10, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=64)',
   'sdpa(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,11,64]:f16, v=cache.vview[2,2,11,64]:f16)',
   '-> start_pos 11',
  ],
 },
 '2/2x64 alibi': {
  'prefill 3 @0': [
   'rope_kv_append(qkv=xqkv[2,3,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=0, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0)',
   '_attend_torch(q=rope_kv_append.out[2,2,3,64]:f16, k=cache.kview[2,2,3,64]:f16, v=cache.vview[2,2,3,64]:f16, first_q_pos=0)',
   '-> start_pos 3',
  ],
  'prefill 2 @3': [
   'rope_kv_append(qkv=xqkv[2,2,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=3, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0)',
   '_attend_torch(q=rope_kv_append.out[2,2,2,64]:f16, k=cache.kview[2,2,5,64]:f16, v=cache.vview[2,2,5,64]:f16, first_q_pos=3)',
   '-> start_pos 5',
  ],
  'decode host': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=5, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0)',
   '_attend_torch(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,6,64]:f16, v=cache.vview[2,2,6,64]:f16, first_q_pos=5)',
   '-> start_pos 6',
  ],
  'decode shared bound 8': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=6, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0, pos_dev=pos[1]:i32)',
   '_attend_torch(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,7,64]:f16, v=cache.vview[2,2,7,64]:f16, first_q_pos=6)',
   '-> start_pos 7',
  ],
  'prefill 2 with device words set': [
   'rope_kv_append(qkv=xqkv[2,2,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=7, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0)',
   '_attend_torch(q=rope_kv_append.out[2,2,2,64]:f16, k=cache.kview[2,2,9,64]:f16, v=cache.vview[2,2,9,64]:f16, first_q_pos=7)',
   '-> start_pos 9',
  ],
  'decode shared': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=9, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0, pos_dev=pos[1]:i32)',
   '_attend_torch(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,10,64]:f16, v=cache.vview[2,2,10,64]:f16, first_q_pos=9)',
   '-> start_pos 10',
  ],
  'decode host again': [
   'rope_kv_append(qkv=xqkv[2,1,384]:f16, k_cache=cache.k[2,16,2,64]:f16, v_cache=cache.v[2,16,2,64]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=10, n_heads=2, n_kv_heads=2, head_dim=64, rotary_dim=0)',
   '_attend_torch(q=rope_kv_append.out[2,2,1,64]:f16, k=cache.kview[2,2,11,64]:f16, v=cache.vview[2,2,11,64]:f16, first_q_pos=10)',
   '-> start_pos 11',
  ],
 },
 'requests': {
  'extend fp16 S 3 max_end 9': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32)',
   'prefill_attention_rows(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32, max_end=9)',
   '-> start_pos 5',
  ],
  'extend fp16 max_end 0': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32)',
   '-> start_pos 5',
  ],
  'extend fp16 max_end 16': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32)',
   'prefill_attention_rows(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32, max_end=16)',
   '-> start_pos 5',
  ],
  'extend fp16 alibi S 3 max_end 9': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32)',
   'prefill_attention_rows(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32, max_end=9, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 5',
  ],
  'extend fp16 alibi max_end 0': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32)',
   '-> start_pos 5',
  ],
  'extend fp16 alibi max_end 16': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[1,1]:f32, sin=sin[1,1]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=0, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32)',
   'prefill_attention_rows(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32, max_end=16, alibi_slopes=alibi.slopes[2]:f32)',
   '-> start_pos 5',
  ],
  'extend fp8 S 3 max_end 9': [
   'rope_kv_append(qkv=xqkv[2,3,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32, count_rows=count_rows[2]:i32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=9, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=9, batch=2)',
   'prefill_attention_rows(q=rope_kv_append.out[2,3,2,128]:f16, k_cache=kv_dequant_fp8.out[2,9,1,128]:f16, v_cache=kv_dequant_fp8.out[2,9,1,128]:f16, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32, max_end=9)',
   '-> start_pos 5',
  ],
  'extend fp8 max_end 0': [
   'rope_kv_append(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32, count_rows=count_rows[2]:i32)',
   '-> start_pos 5',
  ],
  'extend fp8 max_end 16': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:u8, v_cache=cache.v[2,16,1,128]:u8, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32, k_scale=k_scale[2,16,1]:f32, v_scale=v_scale[2,16,1]:f32, count_rows=count_rows[2]:i32)',
   'kv_dequant_fp8(cache=cache.k[2,16,1,128]:u8, scales=k_scale[2,16,1]:f32, n=16, batch=2)',
   'kv_dequant_fp8(cache=cache.v[2,16,1,128]:u8, scales=v_scale[2,16,1]:f32, n=16, batch=2)',
   'prefill_attention_rows(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=kv_dequant_fp8.out[2,16,1,128]:f16, v_cache=kv_dequant_fp8.out[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, count_rows=count_rows[2]:i32, max_end=16)',
   '-> start_pos 5',
  ],
  'verify T 2': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32)',
   'verify_attention_rows(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, max_len=16)',
   '-> start_pos 5',
  ],
  'verify T 8': [
   'rope_kv_append(qkv=xqkv[2,8,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32)',
   'verify_attention_rows(q=rope_kv_append.out[2,8,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, max_len=16)',
   '-> start_pos 5',
  ],
  'verify T 2 bound 4': [
   'rope_kv_append(qkv=xqkv[2,2,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32)',
   'verify_attention_rows(q=rope_kv_append.out[2,2,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, max_len=4)',
   '-> start_pos 5',
  ],
  'verify T 8 bound 4': [
   'rope_kv_append(qkv=xqkv[2,8,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=0, n_heads=2, n_kv_heads=1, head_dim=128, rotary_dim=128, pos_rows=pos_rows[2]:i32)',
   'verify_attention_rows(q=rope_kv_append.out[2,8,2,128]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, pos_rows=pos_rows[2]:i32, max_len=8)',
   '-> start_pos 5',
  ],
  'decode rows after verify': [
   'decode_attention_rope(qkv=xqkv[2,1,512]:f16, k_cache=cache.k[2,16,1,128]:f16, v_cache=cache.v[2,16,1,128]:f16, cos=cos[16,64]:f32, sin=sin[16,64]:f32, start_pos=5, n_heads=2, n_kv_heads=1, max_len=4, pos_rows=pos_rows[2]:i32)',
   '-> start_pos 6',
  ],
 },
}


if __name__ == "__main__":  # prints EXPECTED (run on the commit before the change; see the module docstring)
    r = Recorder()
    attn_mod.ops, attn_mod.F = r, SimpleNamespace(scaled_dot_product_attention=r.sdpa)
    print("EXPECTED = {")
    for case, calls in record_all(r).items():
        print(f" {case!r}: {{")
        for call, lines in calls.items():
            print(f"  {call!r}: [\n" + "".join(f"   {line!r},\n" for line in lines) + "  ],")
        print(" },")
    print("}")
