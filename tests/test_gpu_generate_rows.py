"""GraphedDecoder.generate with per-row arguments on the committed tiny-Llama checkpoint (MI355X, "gemv" layout, batch 3,
max_seq_len 64): sequences of equal values against the scalar call, mixed rows against one scalar call per row, a second turn
with extend=True, left-padded prompts, and the refusals.  Every comparison is on ids and exact: the rows of this model do not
see each other, the per-row attention forms are pinned bitwise to the shared ones and the rows sampler to the shared sampler."""
import pytest
import torch

from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
B, P = 3, 6


@pytest.fixture(scope="module")
def dec():
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    model, _ = load_quantized(skeleton(), ckpt("gemv"), device="cuda")
    return GraphedDecoder(fuse_llama(model, max_seq_len=64), batch=B, buckets=(12, 24))


def _ids(width, shift=0):
    """three different rows of `width` ids cut from the golden prompt ids"""
    flat = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"]).reshape(-1)
    cols = torch.arange(width)
    return torch.stack([flat[(cols + 3 * r + shift) % flat.numel()] for r in range(B)]).long().cuda()


def _vocab(dec):
    return int(dec.lm.model.vocab_size)


MIXED = {"do_sample": [False, True, True], "temperature": [1.0, 0.7, 1.3], "top_k": [0, 20, 0], "top_p": [1.0, 0.9, 0.8],
         "seed": [3, 11, 12], "max_new_tokens": [3, 9, 6], "repetition_penalty": [1.0, 1.3, 1.0], "min_new_tokens": [0, 2, 0]}


def _scalars(args, r):
    return {k: v[r] for k, v in args.items()}


def _real(new, eos, limit):
    """a row's own tokens: up to and including its first EOS id, `limit` at the most"""
    new = new[:limit]
    hit = [i for i, t in enumerate(new) if t in eos]
    return new[:hit[0] + 1] if hit else new


def _check_rows(out, scalar_outs, args, eos_rows, width):
    """row r of `out` = row r of the scalar call with row r's values up to that row's end, its own pad after it"""
    new = out[:, width:].cpu().tolist()
    longest = 0
    for r in range(B):
        want = _real(scalar_outs[r][r, width:].cpu().tolist(), eos_rows[r], args["max_new_tokens"][r])
        assert new[r][:len(want)] == want, (r, new[r], want)
        assert new[r][len(want):] == [eos_rows[r][0]] * (len(new[r]) - len(want)), (r, new[r])
        longest = max(longest, len(want))
    assert out.shape[1] == width + longest


def test_sequences_of_equal_values_equal_the_scalar_call(dec):
    ids = _ids(P)
    scalar = dec.generate(ids, max_new_tokens=8, do_sample=True, temperature=0.7, top_p=0.9, seed=1)
    families = [sorted(f) for f in (dec.gen_graphs, dec.row_gen_graphs, dec.proc_gen_graphs, dec.row_proc_gen_graphs)]
    rows = dec.generate(ids, max_new_tokens=8, do_sample=[True] * 3, temperature=[0.7] * 3, top_p=[0.9] * 3, seed=[1] * 3)
    assert rows.dtype == torch.int64 and torch.equal(rows, scalar)
    assert sorted(dec.rows_gen_graphs) == [12, 24]              # one family of its own, and the existing ones as they were
    assert families == [sorted(f) for f in (dec.gen_graphs, dec.row_gen_graphs, dec.proc_gen_graphs, dec.row_proc_gen_graphs)]
    scalar = dec.generate(ids, max_new_tokens=8)
    rows = dec.generate(ids, max_new_tokens=[8, 8, 8], do_sample=[False] * 3)
    assert torch.equal(rows, scalar)


def test_mixed_rows_equal_one_scalar_call_per_row(dec):
    ids = _ids(P, shift=1)
    V = _vocab(dec)
    eos_rows = [[V - 1], [V - 2, 5], [V - 3]]
    out = dec.generate(ids, eos_token_id=eos_rows, check_every=4, **MIXED)
    assert torch.equal(out[:, :P], ids)
    scalar = [dec.generate(ids, eos_token_id=eos_rows[r], **_scalars(MIXED, r)) for r in range(B)]
    _check_rows(out, scalar, MIXED, eos_rows, P)
    assert out.shape[1] > P + 3 and set(out[0, P + 3:].cpu().tolist()) == {V - 1}   # row 0 past its own limit: its own pad


def test_extend_restarts_every_rows_token_index(dec):
    ids1, ids2 = _ids(P, shift=2), _ids(4, shift=7)
    V = _vocab(dec)
    eos_rows = [[V - 1], [V - 2], [V - 3]]
    turn1 = {"do_sample": [True, False, True], "temperature": [0.8, 1.0, 1.2], "seed": [5, 6, 7], "max_new_tokens": [3, 5, 4],
             "repetition_penalty": [1.0, 1.3, 1.0], "min_new_tokens": [0, 0, 0], "top_k": [0, 0, 10], "top_p": [1.0, 1.0, 1.0]}
    turn2 = dict(turn1, max_new_tokens=[6, 4, 5], min_new_tokens=[2, 0, 3], seed=[8, 9, 10])
    dec.generate(ids1, eos_token_id=eos_rows, **turn1)
    out = dec.generate(ids2, eos_token_id=eos_rows, extend=True, **turn2)
    assert torch.equal(out[:, :4], ids2)
    scalar = []
    for r in range(B):
        dec.generate(ids1, eos_token_id=eos_rows[r], **_scalars(turn1, r))
        scalar.append(dec.generate(ids2, eos_token_id=eos_rows[r], extend=True, **_scalars(turn2, r)))
    _check_rows(out, scalar, turn2, eos_rows, 4)


def test_left_padded_prompts_with_per_row_arguments(dec):
    ids = _ids(P, shift=4)
    mask = torch.ones((B, P), dtype=torch.int64)
    mask[1, :2] = 0
    mask[2, :1] = 0
    V = _vocab(dec)
    eos_rows = [[V - 1], [V - 2, 5], [V - 3]]
    out = dec.generate(ids, attention_mask=mask, eos_token_id=eos_rows, **MIXED)
    scalar = [dec.generate(ids, attention_mask=mask, eos_token_id=eos_rows[r], **_scalars(MIXED, r)) for r in range(B)]
    _check_rows(out, scalar, MIXED, eos_rows, P)


def test_refusals_launch_nothing(dec):
    ids = _ids(P)
    dec.generate(ids, max_new_tokens=2)
    before = (dec.position, dec.positions, dict(dec.rows_gen_graphs), dict(dec.spec_graphs), dec.tail)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, temperature=[1.0, 0.5, 1.0], draft_tokens=3)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=[4, 4], do_sample=False)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, eos_token_id=[[1], [2]])
    assert (dec.position, dec.positions, dict(dec.rows_gen_graphs), dict(dec.spec_graphs), dec.tail) == before
