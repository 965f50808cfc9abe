"""Speculative decoding in GraphedDecoder (verify / advance_rows, generate(draft_tokens=K)) on the committed tiny-Llama checkpoints.

Measured on MI355X (the shares of positions the margin rule leaves out are in the tests' docstrings): with prompt-lookup drafts the
speculative text equalled the plain greedy text token for token in every case run here; a prompt that is one short n-gram repeated
needed 9 .. 21 replays for 32 tokens at draft_tokens=3 (the random tiny model continues some repeats and not others)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
VERSIONS = ["gemm", "gemv", "gemv_fast"]
TOL = 2e-2   # relative to the logit range: the checkpoint-logit tests' tolerance (test_gpu_ragged_generate.py)


def _decoder(version, batch, max_seq_len=64, **kw):
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    model, _ = load_quantized(skeleton(), ckpt(version), device="cuda")
    lm = fuse_llama(model, max_seq_len=max_seq_len, **kw)
    return GraphedDecoder(lm, batch=batch, buckets=(12, 24))


def _prompts(lengths):
    ids = golden("tiny_llama_awq_gemm_outputs")["input_ids"]
    return [torch.from_numpy(ids[i % ids.shape[0], :n].copy()) for i, n in enumerate(lengths)]


def _left_padded(prompts, pad=0):
    S = max(len(p) for p in prompts)
    ids = torch.full((len(prompts), S), pad, dtype=torch.int64)
    mask = torch.zeros((len(prompts), S), dtype=torch.int64)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = p
        mask[b, S - len(p):] = 1
    return ids.cuda(), mask.cuda()


def _hand_loop(dec, ids, mask, toks):
    """prefill + one plain dec.step per column of toks [B, n - 1]: the logits [B, V] (float64) at every token index"""
    logits = dec.prefill(ids, attention_mask=mask)
    if mask is not None:
        last = mask.shape[1] - 1 - mask.flip(1).argmax(1)
        first = logits[torch.arange(ids.shape[0]), last]
    else:
        first = logits[:, -1]
    out = [first.double().cpu().numpy()]
    for i in range(toks.shape[1]):
        out.append(dec.step(toks[:, i:i + 1].cuda())[:, 0].double().cpu().numpy())
    return out


def _plain_run(dec, ids, mask, n):
    """greedy tokens [B, n] of the plain path and its per-step logits"""
    out = dec.generate(ids, max_new_tokens=n, attention_mask=mask).cpu()
    new = out[:, ids.shape[1]:]
    return new, _hand_loop(dec, ids, mask, new[:, :-1])


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("T", [2, 4, 8])
def test_verify_is_a_step(version, T):
    """verify on [last, d1 .. dK], the d's a plain greedy run's tokens: the logits of every slot are that run's per-step logits,
    and after advance_rows with mixed counts a following plain step matches too -- rejected rows leave no trace."""
    lengths = [3, 7, 11]
    ids, mask = _left_padded(_prompts(lengths))
    dec = _decoder(version, 3)
    n = 2 * T + 2
    new, plain = _plain_run(dec, ids, mask, n)
    rng = max(np.abs(x).max() for x in plain)
    dec.prefill(ids, attention_mask=mask)
    got = dec.verify(new[:, :T].cuda()).double().cpu().numpy()        # tokens 1 .. T -> the logits of tokens 2 .. T + 1
    assert dec.positions == lengths and sorted(dec.verify_graphs) == [(24, T)] and dec.spec_graphs == {}
    for j in range(T):
        assert np.abs(got[:, j] - plain[1 + j]).max() <= TOL * rng, j
    counts = [1, T, max(1, T // 2)]
    dec.advance_rows(counts)
    assert dec.positions == [p + c for p, c in zip(lengths, counts)]
    nxt = torch.stack([new[b, c] for b, c in enumerate(counts)]).view(-1, 1)       # row b continues after its count
    step = dec.step(nxt.cuda())[:, 0].double().cpu().numpy()
    for b, c in enumerate(counts):
        assert np.abs(step[b] - plain[1 + c][b]).max() <= TOL * rng, b
    with pytest.raises(RuntimeError):
        dec.advance_rows(counts)
    # a second verify from mixed positions, drafts from the plain run again: every row could advance T where the margins allow
    toks = torch.stack([new[b, c + 1:c + 1 + T] for b, c in enumerate(counts)])
    got = dec.verify(toks.cuda()).double().cpu().numpy()
    for b, c in enumerate(counts):
        for j in range(T):
            want = plain[c + 2 + j][b]
            assert np.abs(got[b, j] - want).max() <= TOL * rng, (b, j)
            top = np.sort(want)[-2:]
            if top[1] - top[0] > TOL * rng:                        # the acceptance rule accepts draft j + 1
                assert int(np.argmax(got[b, j])) == int(new[b, c + 2 + j]), (b, j)


def _teacher_forced(version, out, ids, mask, n_new, B):
    """each emitted token must be the argmax of the plain logits wherever their top-2 margin exceeds TOL x range (_check_row's rule);
    returns the share of positions the rule leaves out"""
    dec = _decoder(version, B)
    new = out[:, ids.shape[1]:]
    plain = _hand_loop(dec, ids, mask, new[:, :-1])
    skipped = total = 0
    for t in range(new.shape[1]):
        for b in range(B):
            if t >= n_new[b]:
                continue
            lg = plain[t][b]
            top = np.sort(lg)[-2:]
            total += 1
            if top[1] - top[0] > TOL * np.abs(lg).max():
                assert int(new[b, t]) == int(np.argmax(lg)), (t, b)
            else:
                skipped += 1
    return skipped / total


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_speculation_does_not_change_the_text(version, K, ragged, B):
    """generate(draft_tokens=K), teacher-forced through plain steps.  Condition: the margin rule leaves out at most a quarter of
    the positions.  The share is a property of the prompt's plain logits (it is the same for every K and layout).  Measured on
    MI355X, 24 new tokens: batch of 1 (9 tokens, masked or not) 0.167; batch of 3, 9 tokens each 0.167 .. 0.236;
    batch of 3 with 9 / 4 / 12 tokens behind a mask 0.181.  The first golden prompt cut at 8 tokens has 7 of its 24 positions
    below the margin (0.292) and is therefore not used as a batch of one; cut at 9 tokens it has 4 (0.167)."""
    lengths = [9, 4, 12][:B] if ragged else [9] * B
    prompts = _prompts(lengths)
    ids, mask = _left_padded(prompts) if ragged else (torch.stack(prompts).cuda(), None)
    n = 24
    dec = _decoder(version, B)
    out = dec.generate(ids, max_new_tokens=n, draft_tokens=K, attention_mask=mask).cpu()
    assert torch.equal(out[:, :ids.shape[1]], ids.cpu()) and out.shape == (B, ids.shape[1] + n)
    assert dec.last_spec["new_tokens"] == [n] * B and 1 <= dec.last_spec["replays"] <= n - 1
    assert dec.positions == [L + n - 1 for L in lengths]
    assert all(k[1] == K + 1 for k in dec.spec_graphs) and dec.spec_graphs
    assert not (dec.graphs or dec.gen_graphs or dec.row_graphs or dec.row_gen_graphs or dec.proc_gen_graphs
                or dec.row_proc_gen_graphs or dec.verify_graphs)
    share = _teacher_forced(version, out, ids, mask, [n] * B, B)
    print(f"{version} K {K} ragged {ragged} B {B}: replays {dec.last_spec['replays']}, margin rule left out {share:.3f}")
    assert share <= 0.25


@pytest.mark.parametrize("version", VERSIONS)
def test_drafts_are_accepted_on_a_repeating_prompt(version):
    """a prompt that is one short n-gram repeated: prompt lookup finds drafts; where the model continues the repeat, fewer replays
    than tokens.  Asserted over a handful of n-grams: at least one of them must save a replay."""
    saved = []
    for gram in ([5, 9], [17, 3, 40], [1, 2], [33, 33, 8], [12], [50, 7, 21, 4]):
        ids = torch.tensor([(gram * 12)[:12]], dtype=torch.int64).cuda()
        dec = _decoder(version, 1)
        n = 32
        out = dec.generate(ids, max_new_tokens=n, draft_tokens=3, draft_ngram=3).cpu()
        plain = dec.generate(ids, max_new_tokens=n).cpu()
        share = _teacher_forced(version, out, ids, None, [n], 1)
        saved.append((n - 1) - dec.last_spec["replays"])
        print(f"{version} gram {gram}: replays {dec.last_spec['replays']} for {n} tokens, left out {share:.3f}, "
              f"equal to the plain run: {bool(torch.equal(out, plain))}")
    assert max(saved) > 0, saved


def test_eos_inside_an_accepted_run_and_budget():
    ids, mask = _left_padded(_prompts([4, 9]))
    S = ids.shape[1]
    dec = _decoder("gemm", 2)
    free = dec.generate(ids, max_new_tokens=20, draft_tokens=3, attention_mask=mask).cpu()
    assert free.shape == (2, S + 20)
    eos = int(free[0, S + 5])
    first = [free[b, S:].tolist().index(eos) if eos in free[b, S:].tolist() else None for b in range(2)]
    out = dec.generate(ids, max_new_tokens=20, draft_tokens=3, eos_token_id=eos, pad_token_id=63, attention_mask=mask,
                       check_every=2).cpu()
    new = out[:, S:]
    assert torch.equal(out[:, :S], ids.cpu())
    for b in range(2):
        if first[b] is None:
            assert new[b].tolist()[:20] == free[b, S:].tolist()
        else:
            assert new[b, :first[b] + 1].tolist() == free[b, S:S + first[b] + 1].tolist()
            assert (new[b, first[b] + 1:] == 63).all()
            assert dec.last_spec["new_tokens"][b] == first[b] + 1
    want_cols = max(20 if f is None else f + 1 for f in first)
    assert new.shape[1] == want_cols
    # budgets that end inside a step: never exceeded
    for n in (1, 2, 3, 6):
        o = dec.generate(ids, max_new_tokens=n, draft_tokens=7, attention_mask=mask).cpu()
        assert o.shape == (2, S + n) and torch.equal(o[:, S:], free[:, S:S + n])
        assert dec.last_spec["new_tokens"] == [n, n]


def test_default_path_creates_nothing_and_refusals():
    ids = torch.stack(_prompts([6, 6])).cuda()
    dec = _decoder("gemv", 2)
    dec.generate(ids, max_new_tokens=4)
    assert dec.spec_graphs == {} and dec.verify_graphs == {} and dec._spec == {} and dec.last_spec is None
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, do_sample=True, temperature=0.8)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, repetition_penalty=1.2)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, min_new_tokens=2)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, draft_tokens=8)
    with pytest.raises(ValueError):   # no window roll: prompt + max_new_tokens + T <= max_seq_len
        dec.generate(ids, max_new_tokens=55, draft_tokens=3)
    dec.generate(ids, max_new_tokens=4, draft_tokens=3, do_sample=True, temperature=0.0)   # greedy by temperature: allowed
    dec8 = _decoder("gemv", 2, kv_cache_dtype="fp8")
    with pytest.raises(NotImplementedError, match="fp8"):
        dec8.generate(ids, max_new_tokens=4, draft_tokens=3)
    with pytest.raises(NotImplementedError, match="fp8"):
        dec8.prefill(ids)
        dec8.verify(ids[:, :3])
