"""The host side of prefill at per-row positions: what a generate call leaves per row (ragged.generate_tail), the mask parsing of
GraphedDecoder.extend (ragged.mask_runs_extend) and the three new symbols in header, library and ctypes table."""
import ctypes
import os
import re

import pytest
import torch

from autoawq_amd import _lib
from autoawq_amd.modules.fused.ragged import generate_tail, mask_runs, mask_runs_extend, pack_ids, unpack_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["awq_prefill_attention_rows", "awq_rope_kv_append_rows_n", "awq_rope_kv_append_rows_n_fp8"]
EOS, PAD = 9, 0


def test_tail_without_eos():
    # n = 4 tokens sampled, 3 of them fed: the cache holds the prompt + 3, the 4th is owed
    ring = [[11, 12, 13, 14], [21, 22, 23, 24]]
    assert generate_tail([5, 2], ring, [], 4) == ([8, 5], [14, 24])
    assert generate_tail([5, 2], ring, [EOS], 4) == ([8, 5], [14, 24])
    assert generate_tail([5, 2], torch.tensor(ring), [EOS], 4) == ([8, 5], [14, 24])


def test_tail_eos_at_the_last_step():
    # the EOS was emitted and never fed: it is the pending token, the cache ends before it
    ring = [[11, 12, EOS], [21, 22, 23]]
    assert generate_tail([4, 4], ring, [EOS], 3) == ([6, 6], [EOS, 23])


def test_tail_eos_earlier_with_pads_fed():
    # row 0: 11, EOS real and fed, then pads fed (dropped); row 1 finishes on token 1; row 2 never does; a second EOS id
    ring = [[11, EOS, PAD, PAD, PAD], [EOS, PAD, PAD, PAD, PAD], [31, 32, 33, 34, 35], [41, 42, 7, PAD, PAD]]
    assert generate_tail([3, 6, 1, 2], ring, [EOS, 7], 5) == ([5, 7, 5, 5], [None, None, 35, None])
    # pad == EOS (the default pad): the first one is the real one
    ring = [[11, EOS, EOS, EOS]]
    assert generate_tail([3], ring, [EOS], 4) == ([5], [None])
    # the ring may be longer than n (its capacity): only the first n columns count
    assert generate_tail([3], [[11, 12, 13, EOS, 99]], [EOS], 3) == ([5], [13])


def test_tail_single_token():
    # n = 1: nothing was fed; the one token is owed whether it is an EOS or not
    assert generate_tail([7, 3], [[11], [EOS]], [EOS], 1) == ([7, 3], [11, EOS])


def test_tail_idle_rows_and_bad_rings():
    # a row that started finished emitted pads only: nothing real, nothing owed -- even where the pad looks like a token
    assert generate_tail([7, 3], [[5, 5, 5], [11, 12, 13]], [], 3, idle=[0]) == ([7, 5], [None, 13])
    with pytest.raises(ValueError):
        generate_tail([7], [[1, 2]], [], 3)
    with pytest.raises(ValueError):
        generate_tail([7], [[]], [], 0)


def test_relaxed_mask_parsing():
    ids_shape = (4, 5)
    m = torch.tensor([[0, 0, 1, 1, 1], [0, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 1, 1, 1]])
    assert mask_runs_extend(m, ids_shape) == ([2, 0, 0, 0], [3, 0, 2, 5])
    assert mask_runs_extend(m.bool(), ids_shape) == ([2, 0, 0, 0], [3, 0, 2, 5])
    with pytest.raises(ValueError):   # the strict parsing is unchanged: an empty row is refused there
        mask_runs(m, ids_shape)
    assert mask_runs_extend(m[[0, 2, 3]], (3, 5)) == mask_runs(m[[0, 2, 3]], (3, 5))
    assert mask_runs_extend(torch.zeros((2, 3), dtype=torch.int64), (2, 3)) == ([0, 0], [0, 0])
    for bad, shape in [(m, (4, 6)), (m.float(), ids_shape), (m * 2, ids_shape), (torch.tensor([[1, 0, 1, 0, 0]]), (1, 5)),
                       (torch.tensor([[0, 1, 0, 0, 1]]), (1, 5))]:
        with pytest.raises(ValueError):
            mask_runs_extend(bad, shape)


def test_rows_without_tokens_pack_and_unpack():
    """GraphedDecoder.extend packs a row without tokens as if it had one (its count stays 0) and unpacks by the real lengths"""
    ids = torch.arange(20).view(4, 5)
    starts, lengths = [2, 0, 0, 0], [3, 0, 2, 5]
    packed = pack_ids(ids, starts, [max(n, 1) for n in lengths])
    assert packed.shape == (4, 5) and packed[0, :3].tolist() == [2, 3, 4] and packed[2, :2].tolist() == [10, 11]
    back = unpack_rows(packed.unsqueeze(-1), starts, lengths, 5)[..., 0]
    assert back[0, 2:].tolist() == [2, 3, 4] and back[2, :2].tolist() == [10, 11] and back[3].tolist() == ids[3].tolist()


def test_new_symbols_in_header_library_and_table():
    header = open(os.path.join(ROOT, "include", "awq_hip.h")).read()
    for name in NEW:
        assert re.search(r"AWQ_EXPORT\s+int\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        m = re.search(r"AWQ_EXPORT\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    if not _lib.available():
        import __graft_entry__

        __graft_entry__.build()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(h, name), f"libawq_hip.so does not export {name}"
    # host-side validation only (nothing is launched): the rows form refuses what the shared form refuses
    L = _lib.lib()
    n = [None] * 6
    assert L.awq_prefill_attention_rows(*n, 8, 1, 8, 4, 2, 128, 64, 1.0, 0.0, None, None) == -6                # NULL
    assert L.awq_prefill_attention(*n[:4], 1, 8, 4, 2, 128, 64, 0, 1.0, 0.0, None, None) == -6
    assert L.awq_prefill_attention_rows(*n, 8, -1, 8, 4, 2, 128, 64, 1.0, 0.0, None, None) == -1
    assert L.awq_rope_kv_append_rows_n(*[None] * 8, 0, 8, 4, 2, 128, 128, 64, None) == 0                       # B == 0
    assert L.awq_rope_kv_append_rows_n(*[None] * 8, 1, 8, 4, 2, 128, 128, 64, None) == -6
    assert L.awq_rope_kv_append_rows_n_fp8(*[None] * 10, 1, 8, 4, 2, 128, 128, 64, None) == -6
