"""Host side of prompts of different lengths (modules/fused/ragged.py, GraphedDecoder's attention_mask): mask validation,
packing the real tokens to positions 0 .. L_b - 1 and back, and the C ABI of the per-row decode kernels."""
import os
import re

import pytest
import torch

from autoawq_amd.modules.fused.ragged import mask_runs, pack_ids, unpack_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_left_right_and_no_padding():
    m = torch.tensor([[0, 0, 1, 1, 1], [1, 1, 0, 0, 0], [1, 1, 1, 1, 1], [0, 1, 1, 0, 0]])
    starts, lengths = mask_runs(m, (4, 5))
    assert starts == [2, 0, 0, 1] and lengths == [3, 2, 5, 2]
    assert mask_runs(m.bool(), (4, 5)) == (starts, lengths)
    ids = torch.arange(20).view(4, 5)
    packed = pack_ids(ids, starts, lengths)
    # real tokens first, then the row's last real token repeated
    assert packed.tolist() == [[2, 3, 4, 4, 4], [5, 6, 6, 6, 6], [10, 11, 12, 13, 14], [16, 17, 17, 17, 17]]
    logits = torch.randn(4, 5, 7)
    back = unpack_rows(logits, starts, lengths, 5)
    for b, (s, n) in enumerate(zip(starts, lengths)):
        assert torch.equal(back[b, s:s + n], logits[b, :n])


def test_positions_match_transformers_convention():
    m = torch.tensor([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1]])
    starts, lengths = mask_runs(m, m.shape)
    pos = (m.cumsum(1) - 1)
    for b, (s, n) in enumerate(zip(starts, lengths)):   # packed column i is the token at position i
        assert pos[b, s:s + n].tolist() == list(range(n))


@pytest.mark.parametrize("mask,shape,what", [
    ([[1, 1, 1], [0, 0, 0]], (2, 3), "no ones"),
    ([[1, 0, 1], [1, 1, 1]], (2, 3), "contiguous"),
    ([[0, 1, 0, 1]], (1, 4), "contiguous"),
    ([[1, 1, 1]], (1, 4), "shape"),
    ([[1, 2, 1]], (1, 3), "0 and 1"),
    ([[0.0, 1.0]], (1, 2), "integers"),
])
def test_rejected_masks(mask, shape, what):
    with pytest.raises(ValueError, match=what):
        mask_runs(torch.tensor(mask), shape)


def test_row_longer_than_the_window_is_rejected():
    m = torch.ones(2, 20, dtype=torch.int64)
    m[0, :5] = 0
    with pytest.raises(ValueError, match="cache window"):
        mask_runs(m, m.shape, max_len=16)
    assert mask_runs(m, m.shape, max_len=20)[1] == [15, 20]


def _header_args(name):
    with open(os.path.join(ROOT, "include", "awq_hip.h")) as f:
        text = f.read()
    m = re.search(r"AWQ_EXPORT int " + name + r"\(([^;]*)\);", text)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype(decl):
    from ctypes import c_float, c_int64, c_size_t, c_void_p

    if "*" in decl:
        return c_void_p
    return {"int64_t": c_int64, "float": c_float, "size_t": c_size_t}[decl.split()[0]]


@pytest.mark.parametrize("name,shared,rows_arg", [("awq_rope_kv_append_rows", "awq_rope_kv_append", "pos_rows"),
                                                  ("awq_decode_attention_rows", "awq_decode_attention_ex", "len_rows"),
                                                  ("awq_decode_attention_rope_rows", "awq_decode_attention_rope", "pos_rows")])
def test_abi_table_has_the_per_row_entry_points(name, shared, rows_arg):
    from autoawq_amd import _lib

    args = _header_args(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert [_ctype(a) for a in args] == argtypes
    assert any(a.replace(" ", "").endswith("int32_t*" + rows_arg) for a in args)
    # the shared form's arguments, with its device word replaced by the [B] array and its host scalar dropped
    drop = {"start_pos", "seq_len"}
    want = [a.replace("pos_dev", rows_arg).replace("len_dev", rows_arg) for a in _header_args(shared)
            if a.split()[-1].lstrip("*") not in drop]
    assert args == want


def _tail_restated(lengths, ring, eos, n, idle):
    """generate_tail's docstring, restated on its own: real = the row's tokens up to and including its first EOS id (n without
    one, 0 for an idle row); the cache holds the prompt and the real tokens that were fed (n - 1 were fed at the most); the last
    real token is pending iff it is token n"""
    cache_rows, pending = [], []
    for b, L in enumerate(lengths):
        row = list(ring[b][:n])
        hits = [i for i, t in enumerate(row) if t in eos]
        real = 0 if b in idle else hits[0] + 1 if hits else n
        cache_rows.append(L + min(real, n - 1))
        pending.append(row[n - 1] if real == n else None)
    return cache_rows, pending


@pytest.mark.parametrize("seed", range(8))
def test_generate_tail_is_the_uniform_case_of_generate_tail_rows(seed):
    """generate_tail(lengths, ring, eos, n, idle) is generate_tail_rows with every row's EOS ids = eos and every budget = n, without
    its third result, and both are the restatement above: a seeded sweep over batch sizes, n = 1 included, rings longer than n,
    idle rows, no / one / several EOS ids."""
    import random

    from autoawq_amd.modules.fused.ragged import generate_tail, generate_tail_rows

    rng = random.Random(seed)
    idle_seen = single = 0
    for _ in range(400):
        B = rng.randint(1, 5)
        n = 1 if rng.random() < 0.2 else rng.randint(2, 9)
        eos = rng.sample(range(6), rng.randint(0, 3))          # a small alphabet: EOS ids hit often, at every column
        ring = [[rng.randrange(6) for _ in range(n + rng.randint(0, 3))] for _ in range(B)]
        lengths = [rng.randint(0, 40) for _ in range(B)]
        idle = [b for b in range(B) if rng.random() < 0.25]
        idle_seen += bool(idle)
        single += n == 1
        want = _tail_restated(lengths, ring, eos, n, idle)
        assert generate_tail_rows(lengths, ring, [eos] * B, [n] * B, n, idle)[:2] == want
        assert generate_tail(lengths, ring, eos, n, idle) == want
        assert generate_tail(lengths, torch.tensor([r[:n] for r in ring]), eos, n, idle=idle) == want
    assert idle_seen > 100 and single > 30
    with pytest.raises(ValueError, match="^generate_tail: row 0"):
        generate_tail([7], [[1, 2]], [], 3)
    with pytest.raises(ValueError, match="^generate_tail_rows: row 0"):
        generate_tail_rows([7], [[1, 2]], [[]], [3], 3)
