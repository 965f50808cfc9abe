"""generate(draft_tokens=K, draft_accept="sampler") on the committed tiny-Llama checkpoints (V = 64, max_seq_len = 64): speculative
decoding with sampling and the logit processors.

The slots sampler asks, per slot, which token the plain sampler would emit there, so the speculative text is the plain sampled
text -- except where the verify step's launch shape rounds the logits differently from a plain step's.  The tests therefore
teacher-force the emitted tokens through plain steps and hold every token to the fp64 restatement of the plain sampler
(tests/spec_sample_ref.py) on those logits wherever its top-2 score gap exceeds 2 TOL range max(p, 1 / p) / temperature: TOL = 2e-2
is the checkpoint-logit tolerance of tests/test_gpu_spec_generate.py, range the largest |logit| of the position's row, p the
repetition penalty (a processed logit moves by at most TOL range max(p, 1 / p), a score by that over the temperature, a gap by twice
it).  The share of positions the rule leaves out is printed by every case; the docstrings hold the measured values."""
import numpy as np
import pytest
import torch

import penalty_ref as pref
import sampling_ref as ref
from test_gpu_spec_generate import TOL, _decoder, _hand_loop, _left_padded, _prompts

pytestmark = pytest.mark.gpu
PROC = dict(repetition_penalty=1.3, min_new_tokens=4)


def _other_families(dec):
    return (dec.graphs or dec.gen_graphs or dec.row_graphs or dec.row_gen_graphs or dec.proc_gen_graphs or dec.row_proc_gen_graphs
            or dec.rows_gen_graphs or dec.lp_gen_graphs or dec.row_lp_gen_graphs or dec.verify_graphs)


def _positions(dec, ids, mask, new, n_new, *, temperature, seed, top_k=0, top_p=1.0, repetition_penalty=1.0, min_new_tokens=0, eos=()):
    """teacher-force `new` through plain steps of `dec`; for every real position yield (b, t, emitted token, the plain logits,
    the restatement's choice on them): the plain sampler at (seed, t, row b), the ids seen = input_ids as passed + the row's
    earlier tokens"""
    plain = _hand_loop(dec, ids, mask, new[:, :-1])
    V = plain[0].shape[1]
    for b in range(new.shape[0]):
        seen = np.zeros(V, dtype=bool)
        seen[ids[b].cpu().numpy()] = True
        for i in range(n_new[b]):
            lg = plain[i][b]
            v = pref.process(lg.astype(np.float16), seen, t=i + 1, repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens,
                             eos_ids=eos)
            yield b, i + 1, int(new[b, i]), lg, v, ref.choose(v, do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p,
                                                               seed=seed, t=i + 1, row=b)
            seen[int(new[b, i])] = True


def _teacher_forced(dec, ids, mask, new, n_new, *, temperature, seed, proc, eos=()):
    """the emitted token is the restatement's wherever its top-2 score gap exceeds 2 TOL range max(p, 1 / p) / temperature;
    returns the share of positions the rule leaves out"""
    p = proc.get("repetition_penalty", 1.0)
    skipped = total = 0
    for b, t, tok, lg, v, (want, keep, s) in _positions(dec, ids, mask, new, n_new, temperature=temperature, seed=seed, eos=eos, **proc):
        top = np.sort(s[np.isfinite(s)])[-2:]
        total += 1
        if top[1] - top[0] > 2 * TOL * np.abs(lg).max() * max(p, 1 / p) / temperature:
            assert tok == want, (b, t, tok, want)
        else:
            skipped += 1
    return skipped / total


@pytest.mark.parametrize("proc", [False, True])
@pytest.mark.parametrize("temperature", [0.7, 1.0])
@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_sampled_speculation_emits_the_plain_sampled_text(B, ragged, K, temperature, proc):
    """Condition: the rule leaves out at most a quarter of the positions (the cap of tests/test_gpu_spec_generate.py).  On the
    committed golden logits the rule leaves out 0.042 at temperature 0.7 and 0.052 at 1.0 (CPU, without the penalty, which widens
    the threshold by 1.3).  Measured on MI355X over the 48 cases (24 new tokens, fewer in a row that emits its EOS id): without the
    processors 0.000 .. 0.083 (0.042 in 9 cases), with them 0.000 .. 0.125 (batch of 1, K = 7, temperature 1.0).  The random
    tiny model accepts no draft on these prompts (23 replays for 24 tokens); the repeating prompts below are where drafts are accepted."""
    lengths = [9, 4, 12][:B] if ragged else [9] * B
    prompts = _prompts(lengths)
    ids, mask = _left_padded(prompts) if ragged else (torch.stack(prompts).cuda(), None)
    S, n, seed = ids.shape[1], 24, 1000 + K
    dec = _decoder("gemm", B)
    kw = dict(max_new_tokens=n, draft_tokens=K, draft_accept="sampler", do_sample=True, temperature=temperature, seed=seed,
              attention_mask=mask)
    eos = ()
    if proc:
        free = dec.generate(ids, **kw, **PROC).cpu()
        eos = (int(free[0, S + 7]),)                           # an id the run emits, past the min_new_tokens window
        kw.update(PROC, eos_token_id=eos[0], pad_token_id=63)
    out = dec.generate(ids, **kw).cpu()
    n_new = dec.last_spec["new_tokens"]
    new = out[:, S:]
    assert torch.equal(out[:, :S], ids.cpu()) and new.shape[1] == max(n_new)
    if proc:
        for b in range(B):
            row = new[b].tolist()
            assert eos[0] not in row[:4]                       # suppressed while t <= min_new_tokens
            first = row.index(eos[0]) + 1 if eos[0] in row[:n_new[b]] else n
            assert n_new[b] == first and all(x == 63 for x in row[n_new[b]:])
        assert n_new[0] <= 8 or eos[0] in free[0, S:S + 4].tolist()
    else:
        assert n_new == [n] * B
    assert 1 <= dec.last_spec["replays"] <= n - 1
    assert dec.positions == [L + c - 1 for L, c in zip(lengths, n_new)]
    assert dec.spec_sample_graphs and all(k[1] == K + 1 for k in dec.spec_sample_graphs)
    assert not (_other_families(dec) or dec.spec_graphs or dec._spec)
    share = _teacher_forced(dec, ids, mask, new, n_new, temperature=temperature, seed=seed, proc=PROC if proc else {}, eos=eos)
    print(f"B {B} ragged {ragged} K {K} temperature {temperature} proc {proc}: replays {dec.last_spec['replays']}, new {n_new}, "
          f"rule left out {share:.3f}")
    assert share <= 0.25


def test_drafts_are_accepted_on_a_repeating_prompt():
    """the repeating n-gram prompts of tests/test_gpu_spec_generate.py with do_sample=True, top_k=1 (the kept set is the argmax, so
    the sampled run is the greedy run): at least one n-gram needs fewer replays than tokens.  Measured on MI355X: 17 / 21 / 15 / 14 /
    9 / 18 replays for 32 tokens."""
    saved = []
    for gram in ([5, 9], [17, 3, 40], [1, 2], [33, 33, 8], [12], [50, 7, 21, 4]):
        ids = torch.tensor([(gram * 12)[:12]], dtype=torch.int64).cuda()
        dec = _decoder("gemm", 1)
        n = 32
        dec.generate(ids, max_new_tokens=n, draft_tokens=3, draft_ngram=3, draft_accept="sampler", do_sample=True, top_k=1, seed=5)
        assert dec.last_spec["new_tokens"] == [n]
        saved.append((n - 1) - dec.last_spec["replays"])
        print(f"gram {gram}: replays {dec.last_spec['replays']} for {n} tokens")
    assert max(saved) > 0, saved


def test_seeds():
    ids, mask = _left_padded(_prompts([9, 4, 12]))
    dec = _decoder("gemm", 3)
    kw = dict(max_new_tokens=24, draft_tokens=3, draft_accept="sampler", do_sample=True, temperature=1.0, attention_mask=mask)
    a = dec.generate(ids, seed=1, **kw).cpu()
    b = dec.generate(ids, seed=1, **kw).cpu()
    c = dec.generate(ids, seed=2, **kw).cpu()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len(dec.spec_sample_graphs) >= 1 and len(dec._spec_sample) == 1    # the second and third call replay the first's graphs


def test_top_k_and_top_p():
    """top_k = 8, top_p = 0.9: the run completes and every emitted token lies in the restatement's kept set on the plain logits,
    widened by the margin m = 2 TOL range: a token whose logit is within m of the smallest kept logit passes (the top-k boundary
    moves by at most that), under top_p' = min(1, top_p e^(m / temperature)) (every mass ratio moves by at most that factor)."""
    ids, mask = _left_padded(_prompts([9, 4, 12]))
    dec = _decoder("gemm", 3)
    n, temperature, seed = 24, 0.8, 3
    out = dec.generate(ids, max_new_tokens=n, draft_tokens=3, draft_accept="sampler", do_sample=True, temperature=temperature, top_k=8,
                       top_p=0.9, seed=seed, attention_mask=mask).cpu()
    assert dec.last_spec["new_tokens"] == [n] * 3
    new = out[:, ids.shape[1]:]
    inside = 0
    for b, t, tok, lg, v, _ in _positions(dec, ids, mask, new, [n] * 3, temperature=temperature, seed=seed):
        m = 2 * TOL * np.abs(lg).max()
        keep = ref.kept_set(v, temperature, 8, min(1.0, 0.9 * np.exp(m / temperature)))
        assert v[tok] >= v[keep].min() - m, (b, t, tok)
        inside += bool(ref.kept_set(v, temperature, 8, 0.9)[tok])
    print(f"top_k 8 top_p 0.9: {inside} of {3 * n} tokens inside the unwidened kept set")


def test_refusals_and_the_greedy_path_is_untouched():
    from autoawq_amd.fuser import fuse_mixtral
    from autoawq_amd.modules.fused.decode import GraphedDecoder
    import test_mixtral

    ids = torch.stack(_prompts([6, 6])).cuda()
    dec = _decoder("gemv", 2)
    kw = dict(max_new_tokens=8, draft_tokens=3, draft_accept="sampler")
    with pytest.raises(ValueError, match="draft_accept"):
        dec.generate(ids, max_new_tokens=8, draft_tokens=3, draft_accept="rejection")
    with pytest.raises(ValueError, match="draft_tokens"):
        dec.generate(ids, max_new_tokens=8, draft_accept="sampler")
    with pytest.raises(ValueError, match="per-row"):
        dec.generate(ids, **kw, do_sample=True, seed=[1, 2])
    with pytest.raises(ValueError, match="per-row"):
        dec.generate(ids, **kw, eos_token_id=[[1], [2]])
    with pytest.raises(ValueError, match="extend"):
        dec.generate(ids, **kw, extend=True)
    with pytest.raises(ValueError, match="logprobs"):
        dec.generate(ids, **kw, logprobs=True)
    with pytest.raises(ValueError):   # no window roll: prompt + max_new_tokens + T <= max_seq_len
        dec.generate(ids, max_new_tokens=55, draft_tokens=3, draft_accept="sampler")
    assert dec._spec_sample == {} and dec.spec_sample_graphs == {} and dec.last_spec is None
    dec8 = _decoder("gemv", 2, kv_cache_dtype="fp8")
    with pytest.raises(NotImplementedError, match="fp8"):
        dec8.generate(ids, **kw, do_sample=True)
    mix = GraphedDecoder(fuse_mixtral(test_mixtral.build().cuda(), max_seq_len=32), batch=2, buckets=(8, 16))
    with pytest.raises(NotImplementedError, match="fuse_mixtral"):
        mix.generate(ids[:, :4] % test_mixtral.V, max_new_tokens=4, draft_tokens=3, draft_accept="sampler", do_sample=True)
    # "argmax" is today's path: its refusals, its graphs, and the same text before and after a "sampler" call on this decoder
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=8, draft_tokens=3, draft_accept="argmax", do_sample=True, temperature=0.8)
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=8, draft_tokens=3, repetition_penalty=1.2)
    before = dec.generate(ids, max_new_tokens=16, draft_tokens=3).cpu()
    graphs = {k: id(v[0]) for k, v in dec.spec_graphs.items()}
    words = {k: v.data_ptr() for k, v in dec._spec[4].items() if isinstance(v, torch.Tensor)}
    assert graphs and dec.spec_sample_graphs == {} and dec._spec_sample == {}
    dec.generate(ids, **kw, do_sample=True, temperature=0.9, seed=4, repetition_penalty=1.2)
    assert dec.spec_sample_graphs and {k: id(v[0]) for k, v in dec.spec_graphs.items()} == graphs
    after = dec.generate(ids, max_new_tokens=16, draft_tokens=3, draft_accept="argmax").cpu()
    assert torch.equal(before, after)
    assert {k: id(v[0]) for k, v in dec.spec_graphs.items()} == graphs and words == {k: v.data_ptr() for k, v in dec._spec[4].items() if isinstance(v, torch.Tensor)}
    # greedy under "sampler" (do_sample=False): the plain greedy text, as under "argmax"
    greedy = dec.generate(ids, max_new_tokens=16, draft_tokens=3, draft_accept="sampler").cpu()
    assert torch.equal(greedy, before)
