"""CPU checks of the sampler's rows form (awq_sample_tokens_rows, csrc/sample.hip): the ctypes struct against the header, the
exported symbol, the per-row packers (broadcast, row order, refusals that name the row, before any device call) and the
entry point's host-side validation against the codes awq_sample_tokens returns for the same arguments."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

_CTYPES = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t}


def _header_struct(name):
    """the fields of a struct of include/awq_hip.h, parsed as tests/test_sampling_penalty_cpu.py does"""
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


def test_rows_args_struct_matches_the_header():
    from autoawq_amd import _lib

    fields = _header_struct("AwqSampleRowsArgs")
    cls = _lib.AwqSampleRowsArgs
    assert [f for f, _ in fields] == [f for f, _ in cls._fields_]

    class FromHeader(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(cls) == ctypes.sizeof(FromHeader) == 160
    for f, _ in fields:
        assert getattr(cls, f).offset == getattr(FromHeader, f).offset, f
    # what AwqSampleArgs carries comes first, at the same offsets; the pinned structs keep their sizes
    shared = _header_struct("AwqSampleArgs")
    assert [f for f, _ in fields[:len(shared)]] == [f for f, _ in shared]
    for f, _ in shared:
        assert getattr(cls, f).offset == getattr(_lib.AwqSampleArgs, f).offset, f
    assert (ctypes.sizeof(_lib.AwqSampleArgs), ctypes.sizeof(_lib.AwqSampleParams), ctypes.sizeof(_lib.AwqSampleProc),
            ctypes.sizeof(_lib.AwqSampleProcArgs)) == (128, 64, 16, 32)


def test_entry_point_exported_and_listed():
    from autoawq_amd import _lib

    assert "awq_sample_tokens_rows" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["awq_sample_tokens_rows"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.AwqSampleRowsArgs)]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "awq_sample_tokens_rows")


# ---- packing ---------------------------------------------------------------------------------------------------------------

def test_scalars_broadcast_to_the_bytes_of_sample_params():
    from autoawq_amd import ops

    cfg = dict(do_sample=True, temperature=0.7, top_k=40, top_p=0.9, seed=2 ** 63 + 5, eos_ids=(3, 9), pad=1)
    one = ops.sample_params(**cfg)
    rows = ops.sample_params_rows(5, **cfg)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (5, 64) and rows.is_contiguous()
    for r in range(5):
        assert torch.equal(rows[r], one)
    proc = ops.sample_proc_params_rows(4, 1.3, 2)
    assert tuple(proc.shape) == (4, 16)
    for r in range(4):
        assert torch.equal(proc[r], ops.sample_proc_params(1.3, 2))
    assert torch.equal(ops.sample_params_rows(2, do_sample=False), torch.stack([ops.sample_params(do_sample=False)] * 2))


def test_per_row_values_land_in_row_order():
    from autoawq_amd import _lib, ops

    ds, T, k, p, seed = [False, True, True], [1.0, 0.5, 1.5], [0, 7, 0], [1.0, 0.9, 0.25], [1, 2 ** 64 - 1, 3]
    eos, pad = [(5,), (), (8, 9, 10)], [None, 4, None]
    rows = ops.sample_params_rows(3, do_sample=ds, temperature=T, top_k=k, top_p=p, seed=seed, eos_ids=eos, pad=pad)
    for r in range(3):
        want = ops.sample_params(do_sample=ds[r], temperature=T[r], top_k=k[r], top_p=p[r], seed=seed[r], eos_ids=eos[r], pad=pad[r])
        assert torch.equal(rows[r], want), r
    q = _lib.AwqSampleParams.from_buffer_copy(bytes(rows[2].numpy()))
    assert (q.seed, q.do_sample, q.n_eos, q.pad, list(q.eos)[:3]) == (3, 1, 3, 8, [8, 9, 10])
    # a mix of scalars and sequences, tensors and tuples as sequences, one EOS tuple for every row
    mixed = ops.sample_params_rows(3, do_sample=True, temperature=torch.tensor(T), top_k=tuple(k), eos_ids=(2, 3))
    for r in range(3):
        assert torch.equal(mixed[r], ops.sample_params(do_sample=True, temperature=T[r], top_k=k[r], eos_ids=(2, 3))), r
    proc = ops.sample_proc_params_rows(3, [1.0, 1.3, 0.5], [0, 4, 1])
    for r, (pen, mn) in enumerate(zip([1.0, 1.3, 0.5], [0, 4, 1])):
        assert torch.equal(proc[r], ops.sample_proc_params(pen, mn)), r
    assert torch.equal(ops.sample_proc_params_rows(2, 1.1, [0, 3])[1], ops.sample_proc_params(1.1, 3))


BAD_PARAMS = [("temperature", [1.0, float("nan"), 1.0], 1), ("top_p", [0.5, 1.0, 0.0], 2), ("top_k", [-1, 0, 0], 0),
              ("eos_ids", [(1,), (2,), tuple(range(9))], 2)]


@pytest.mark.parametrize("name,value,row", BAD_PARAMS, ids=[b[0] for b in BAD_PARAMS])
def test_bad_values_raise_naming_the_row(name, value, row):
    from autoawq_amd import ops

    with pytest.raises(ValueError, match=f"row {row}"):
        ops.sample_params_rows(3, **{"do_sample": True, name: value})
    x = torch.zeros((3, 16), dtype=torch.float16)  # a CPU tensor: a device call would raise AwqHipError, not ValueError
    with pytest.raises(ValueError, match=f"row {row}"):
        ops.sample_tokens_rows(x, **{"do_sample": True, name: value})


def test_bad_processors_raise_naming_the_row():
    from autoawq_amd import ops

    x = torch.zeros((3, 16), dtype=torch.float16)
    for kw, row in (({"repetition_penalty": [1.0, 0.0, 1.0]}, 1), ({"repetition_penalty": [1.0, 1.2, -2.0]}, 2),
                    ({"min_new_tokens": [-1, 0, 0]}, 0)):
        with pytest.raises(ValueError, match=f"row {row}"):
            ops.sample_proc_params_rows(3, **kw)
        with pytest.raises(ValueError, match=f"row {row}"):
            ops.sample_tokens_rows(x, do_sample=False, **kw)
    with pytest.raises(ValueError, match="row 1"):
        ops.sample_tokens_rows(x, do_sample=False, t=[1, 0, 2])
    with pytest.raises(ValueError):  # a penalty without a history, as sample_tokens
        ops.sample_tokens_rows(x, do_sample=False, repetition_penalty=[1.0, 1.3, 1.0])


@pytest.mark.parametrize("name", ["do_sample", "temperature", "top_k", "top_p", "seed", "pad", "eos_ids"])
def test_a_sequence_of_the_wrong_length_is_refused(name):
    from autoawq_amd import ops

    value = [(1,), (2,)] if name == "eos_ids" else [1, 1]
    kw = {"do_sample": True}
    kw[name] = value
    with pytest.raises(ValueError, match="rows"):
        ops.sample_params_rows(3, **kw)
    x = torch.zeros((3, 16), dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.sample_tokens_rows(x, **kw)
    with pytest.raises(ValueError):
        ops.sample_tokens_rows(x, do_sample=False, t=[1, 2])
    with pytest.raises(ValueError):
        ops.sample_proc_params_rows(3, [1.0, 1.0])
    with pytest.raises(ValueError):
        ops.sample_proc_params_rows(3, 1.0, [0, 0, 0, 0])


# ---- host-side validation of the entry point ----------------------------------------------------------------------------------

def _fill(a, B=2, V=100):
    """arguments that pass every check but were never allocated: each case below breaks one of them, so nothing is launched"""
    a.struct_bytes = ctypes.sizeof(a)
    a.flags = 0
    a.logits, a.B, a.V, a.row_stride = 0x10000, B, V, V
    a.params, a.t, a.out, a.out_stride = 0x20000, 0x30000, 0x40000, 1
    a.ring, a.ring_cap, a.finished, a.status = None, 0, None, 0x50000
    a.workspace, a.workspace_bytes, a.stream = 0x60000, 1 << 30, None
    return a


SHARED_CASES = [("struct_bytes", 8, -1), ("B", 0, -3), ("B", 1025, -3), ("V", 0, -3), ("V", (1 << 20) + 1, -3), ("row_stride", 99, -1),
                ("logits", None, -6), ("params", None, -6), ("t", None, -6), ("out", None, -6), ("status", None, -6),
                ("workspace", None, -6), ("ring", 0x70000, -1), ("workspace_bytes", 64, -4), ("workspace", 0x60010, -2),
                ("logits", 0x10001, -2)]


@pytest.mark.parametrize("field,value,code", SHARED_CASES, ids=[f"{f}={v}" for f, v, _ in SHARED_CASES])
def test_entry_point_returns_the_codes_of_the_shared_form(field, value, code):
    from autoawq_amd import _lib

    L = _lib.lib()
    rows, shared = _fill(_lib.AwqSampleRowsArgs()), _fill(_lib.AwqSampleArgs())
    setattr(rows, field, value)
    setattr(shared, field, value)
    assert L.awq_sample_tokens_rows(ctypes.byref(rows)) == L.awq_sample_tokens(ctypes.byref(shared)) == code


def test_entry_point_checks_of_its_own():
    from autoawq_amd import _lib

    L = _lib.lib()
    assert L.awq_sample_tokens_rows(None) == L.awq_sample_tokens(None) == -6
    a = _fill(_lib.AwqSampleRowsArgs())
    a.proc = 0x80000                                       # proc without history
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -6
    a.proc, a.history, a.history_stride = None, 0x90000, 4  # history without proc
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -6
    a.proc, a.history_stride = 0x80000, 3                  # stride < ceil(V / 32), as awq_sample_tokens_ex
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -1
    a.history_stride, a.proc = 4, 0x80008                  # proc 16-byte aligned
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -2
    a.proc, a.history = 0x80000, 0x90002
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -2
    a = _fill(_lib.AwqSampleRowsArgs())
    a.max_new = 0xA0000                                    # the budget latches `finished`: refused without it
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -6
    a.finished, a.max_new = 0xB0000, 0xA0002
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -2
    a.max_new, a.t = 0xA0000, 0x30001
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -2
    a.t, a.params = 0x30000, 0x20004
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -2
    a = _fill(_lib.AwqSampleRowsArgs())
    a.struct_bytes = ctypes.sizeof(_lib.AwqSampleArgs)     # the shared struct's size is not this struct's
    assert L.awq_sample_tokens_rows(ctypes.byref(a)) == -1


def test_generate_refuses_before_any_launch():
    """draft_tokens with a per-row argument, and a sequence of the wrong length: ValueError from the argument checks, which come
    before generate touches the model (a decoder whose model raises on any use)."""
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("generate touched the model: " + name)

    dec = GraphedDecoder.__new__(GraphedDecoder)
    dec.batch, dec.device, dec.lm = 3, torch.device("cpu"), Untouchable()
    ids = torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="draft_tokens"):
        dec.generate(ids, max_new_tokens=4, temperature=[1.0, 0.5, 1.0], draft_tokens=3)
    with pytest.raises(ValueError, match="draft_tokens"):
        dec.generate(ids, max_new_tokens=[4, 4, 4], draft_tokens=3)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, top_k=[1, 2])
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=[4, 4, 4, 4])
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, eos_token_id=[[1], [2]])
    with pytest.raises(ValueError, match="row 1"):
        dec.generate(ids, max_new_tokens=[4, 0, 4])
    with pytest.raises(ValueError, match="row 2"):
        dec.generate(ids, max_new_tokens=4, top_p=[1.0, 1.0, 0.0])
