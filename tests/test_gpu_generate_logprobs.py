"""GraphedDecoder.generate(logprobs=True) and GraphedDecoder.score on the committed tiny-Llama checkpoints (MI355X).

The values are held to the fp64 log-softmax of the logits a hand loop of dec.prefill / dec.step over the generated ids produces
(the loop tests/test_gpu_generate.py uses), within the bound of tests/logprob_bound.py: the step graphs and the generation
graphs record the same launches on the same buffers."""
import numpy as np
import pytest
import torch

import logprob_bound as lb
from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
PAD = 0


def _decoder(version, batch, max_seq_len=32, **kw):
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    model, _ = load_quantized(skeleton(), ckpt(version), device="cuda")
    lm = fuse_llama(model, max_seq_len=max_seq_len, **kw)
    return GraphedDecoder(lm, batch=batch, buckets=(12, 24))


def _prompt(batch, n=6):
    ids = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"]).cuda()
    return ids[:batch, :n] if batch <= ids.shape[0] else ids[:1, :n].repeat(batch, 1)


def _hand_logits(dec, prompt, new, mask=None, per_row=False, first=None):
    """fp16 [B, n, V]: the logits each of the n new tokens was chosen from, by prefill + step over the generated ids.  per_row: the
    steps run at per-row positions, as a call with per-row arguments does; first: token 1's logits where the caller made them."""
    B, n = new.shape
    if first is None:
        logits = dec.prefill(prompt, attention_mask=mask)
        if mask is not None and dec.positions is not None:
            last = mask.shape[1] - 1 - mask.flip(1).argmax(1)
            first = logits[torch.arange(B), last.to(logits.device)]
        else:
            first = logits[:, -1]
            if per_row:
                dec.seek_rows([dec.position] * B)
    rows = [first.reshape(B, -1).cpu().numpy().copy()]
    for i in range(n - 1):
        rows.append(dec.step(new[:, i].reshape(B, 1).cuda())[:, 0].cpu().numpy().copy())
    return np.stack(rows, 1)


def _assert_values(lp, logits, new, real, what):
    """lp [B, n] against the fp64 reference on logits [B, n, V] at ids new [B, n], within the bound, for each row's first real[b]
    slots; exactly 0.0 after them"""
    lp, new = lp.cpu().numpy(), new.cpu().numpy()
    B, n = new.shape
    assert lp.shape == (B, n) and lp.dtype == np.float32, (lp.shape, lp.dtype)
    worst = 0.0
    for b in range(B):
        k = real[b]
        assert (lp[b, k:] == 0.0).all(), (what, b, lp[b])
        if k:
            want, bound = lb.logprob_bound(logits[b, :k], new[b, :k])
            worst = max(worst, lb.assert_logprobs_close(lp[b, :k], want, bound, f"{what}, row {b}"))
            assert (lp[b, :k] < 0.0).all()
    print(f"{what}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("sampled", [False, True])
def test_ids_are_unchanged_and_values_match_the_hand_loop(batch, sampled):
    cfg = {"do_sample": True, "seed": 11, "temperature": 0.9, "top_k": 20, "top_p": 0.9} if sampled else {}
    dec = _decoder("gemm", batch)
    prompt = _prompt(batch)
    plain = dec.generate(prompt, max_new_tokens=10, **cfg)
    assert dec.last_logprobs is None
    out = dec.generate(prompt, max_new_tokens=10, logprobs=True, **cfg)
    assert torch.equal(out, plain)
    lp = dec.last_logprobs
    assert lp.is_cuda and lp.dtype == torch.float32 and lp.shape == (batch, 10)
    new = out[:, 6:]
    _assert_values(lp, _hand_logits(dec, prompt, new), new, [10] * batch, f"batch {batch} sampled {sampled}")
    dec.generate(prompt, max_new_tokens=4, **cfg)
    assert dec.last_logprobs is None                      # a call without logprobs says so


def test_plain_calls_keep_their_graph_families_and_allocate_no_logprob_words():
    dec = _decoder("gemm", 2)
    prompt = _prompt(2)
    dec.generate(prompt, max_new_tokens=10)
    dec.generate(prompt, max_new_tokens=4, repetition_penalty=1.3)
    dec.generate(prompt, max_new_tokens=[3, 4])
    assert sorted(dec.gen_graphs) == [(12, True), (24, True)] and sorted(dec.proc_gen_graphs) == [(12, True)] and sorted(dec.rows_gen_graphs) == [12]
    assert dec.lp_gen_graphs == {} and dec.row_lp_gen_graphs == {}
    assert "lp" not in dec._gen and "lp_slot" not in dec._gen and "lp" not in dec._gen_rows
    assert dec.last_logprobs is None
    dec2 = _decoder("gemm", 1)
    dec2.generate(_prompt(1), max_new_tokens=10)
    assert sorted(dec2.graphs) == [] and sorted(dec2.gen_graphs) == [(12, True), (24, True)]
    ring = dec2._gen["ring"]
    out = dec2.generate(_prompt(1), max_new_tokens=10, logprobs=True)   # the words are added beside the sampler's, which stay
    assert dec2._gen["ring"] is ring and dec2._gen["lp"].shape == ring.shape and dec2._gen["lp_slot"].dtype == torch.int32
    assert sorted(dec2.gen_graphs) == [(12, True), (24, True)] and sorted(dec2.lp_gen_graphs) == [(12, (True, False)), (24, (True, False))]
    assert torch.equal(out, dec2.generate(_prompt(1), max_new_tokens=10))


@pytest.mark.parametrize("check_every", [1, 4])
def test_rows_that_end_at_an_eos_hold_zeros_after_it(check_every):
    dec = _decoder("gemm", 2)
    prompt = _prompt(2)
    free = dec.generate(prompt, max_new_tokens=12).cpu()
    eos = int(free[0, 6 + 2])              # row 0 emits it as its third token
    out = dec.generate(prompt, max_new_tokens=12, eos_token_id=eos, pad_token_id=PAD, check_every=check_every, logprobs=True)
    new = out[:, 6:]
    real = []
    for b in range(2):
        row = new[b].tolist()
        real.append(row.index(eos) + 1 if eos in row else len(row))
    assert real[0] <= 3 and dec.last_logprobs.shape == new.shape
    _assert_values(dec.last_logprobs, _hand_logits(dec, prompt, new), new, real, f"eos, check_every {check_every}")


def test_per_row_budgets_leave_zeros_after_a_rows_own_limit():
    dec = _decoder("gemm", 2)
    prompt = _prompt(2)
    plain = dec.generate(prompt, max_new_tokens=[3, 9], pad_token_id=PAD)
    out = dec.generate(prompt, max_new_tokens=[3, 9], pad_token_id=PAD, logprobs=True)
    assert torch.equal(out, plain) and out.shape == (2, 15)
    assert sorted(dec.row_lp_gen_graphs) == [(12, "rows"), (24, "rows")] and dec.lp_gen_graphs == {}
    new = out[:, 6:]
    lp = dec.last_logprobs
    assert (lp[0, :3] != 0).all() and (lp[0, 3:] == 0).all()
    _assert_values(lp, _hand_logits(dec, prompt, new, per_row=True), new, [3, 9], "max_new_tokens [3, 9]")
    # sampled rows with their own temperatures: the values are still the raw distribution's
    cfg = {"do_sample": [True, False], "temperature": [0.7, 1.0], "seed": [3, 4], "max_new_tokens": 6}
    out = dec.generate(prompt, logprobs=True, **cfg)
    assert torch.equal(out, dec.generate(prompt, **cfg))
    out = dec.generate(prompt, logprobs=True, **cfg)
    _assert_values(dec.last_logprobs, _hand_logits(dec, prompt, out[:, 6:], per_row=True), out[:, 6:], [6, 6], "per-row sampling")


def test_left_padded_prompts_and_the_logit_processors():
    dec = _decoder("gemv", 2)
    ids = _prompt(2, 8).clone()
    mask = torch.ones_like(ids)
    mask[0, :3] = 0
    ids[0, :3] = PAD
    cfg = {"attention_mask": mask, "repetition_penalty": 1.3, "min_new_tokens": 2}
    plain = dec.generate(ids, max_new_tokens=8, **cfg)
    out = dec.generate(ids, max_new_tokens=8, logprobs=True, **cfg)
    assert torch.equal(out, plain)
    assert sorted(k[1] for k in dec.row_lp_gen_graphs) == [(True, True)] * len(dec.row_lp_gen_graphs) and dec.row_lp_gen_graphs
    new = out[:, 8:]
    # the processors change which token is chosen, not the distribution it is scored under
    _assert_values(dec.last_logprobs, _hand_logits(dec, ids, new, mask=mask), new, [8, 8], "left-padded, processors on")


def test_idle_row_and_second_turn_under_extend():
    dec = _decoder("gemv", 2)
    ids2 = torch.tensor([[PAD, PAD], [4, 8]]).cuda()
    mask2 = torch.tensor([[0, 0], [1, 1]]).cuda()
    out = dec.generate(ids2, max_new_tokens=4, attention_mask=mask2, pad_token_id=PAD, extend=True, logprobs=True)
    lp = dec.last_logprobs
    assert lp.shape == (2, 4) and (lp[0] == 0).all() and (lp[1] < 0).all() and (out[0, 2:] == PAD).all()
    # two turns: the second call's values are the second turn's alone
    dec = _decoder("gemv", 2)
    prompt = _prompt(2)
    out1 = dec.generate(prompt, max_new_tokens=5, logprobs=True)
    lp1 = dec.last_logprobs.clone()
    turn2 = _prompt(2, 9)[:, 6:]
    out2 = dec.generate(turn2, max_new_tokens=4, extend=True, logprobs=True)
    lp2 = dec.last_logprobs
    assert lp1.shape == (2, 5) and lp2.shape == (2, 4) and (lp2 < 0).all()
    # the hand loop: a second decoder brought to the same state, token 1's logits from the same extend, then steps
    ref = _decoder("gemv", 2)
    assert torch.equal(ref.generate(prompt, max_new_tokens=5), out1)
    first, _ = ref._first_logits(turn2, None, extend=True)
    new2 = out2[:, 3:]
    _assert_values(lp2, _hand_logits(ref, None, new2, first=first), new2, [4, 4], "second turn")


@pytest.mark.parametrize("case", ["fp8", "roll"])
def test_fp8_cache_and_window_roll(case):
    if case == "fp8":
        dec, n = _decoder("gemv", 2, kv_cache_dtype="fp8"), 10
    else:
        dec, n = _decoder("gemv", 1, max_seq_len=16), 30     # rolls the window, as the hand loop's steps do
    prompt = _prompt(dec.batch)
    plain = dec.generate(prompt, max_new_tokens=n)
    out = dec.generate(prompt, max_new_tokens=n, logprobs=True)
    assert torch.equal(out, plain) and out.shape == (dec.batch, 6 + n)
    if case == "roll":
        assert dec.position < 16
    new = out[:, 6:]
    _assert_values(dec.last_logprobs, _hand_logits(dec, prompt, new), new, [n] * dec.batch, case)


def _spy(monkeypatch):
    from autoawq_amd import ops

    calls, real = [], ops.token_logprobs

    def spy(logits, ids, out=None):
        res = real(logits, ids, out)
        calls.append((logits, ids, res))
        return res

    monkeypatch.setattr(ops, "token_logprobs", spy)
    return calls


@pytest.mark.parametrize("padded", [False, True])
def test_score(monkeypatch, padded):
    from autoawq_amd import ops

    calls = _spy(monkeypatch)
    dec = _decoder("gemm", 2)
    ids = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"]).cuda()[:2, :12].clone()
    mask = None
    if padded:
        mask = torch.ones_like(ids)
        mask[0, :4] = 0
        ids[0, :4] = PAD
    got = dec.score(ids, attention_mask=mask)
    assert got.shape == (2, 12) and got.dtype == torch.float32 and got.is_cuda and len(calls) == 1
    logits, labels, res = calls[0]
    assert logits.shape == (2, 12, 64) and logits.dtype == torch.float16 and labels.shape == (2, 12)
    # the labels: the next token, -1 in the last slot and wherever either side is masked
    want_labels = torch.full((2, 12), -1, dtype=torch.int64)
    want_labels[:, :-1] = ids[:, 1:].cpu()
    if padded:
        want_labels[0, :4] = -1
    assert torch.equal(labels.cpu(), want_labels)
    # the result is the fp64 reference on what the kernel was given, within the bound (prefill need not be reproducible for this)
    want, bound = lb.logprob_bound(logits.reshape(24, 64).cpu().numpy(), labels.reshape(-1).cpu().numpy())
    lb.assert_logprobs_close(res.cpu().numpy(), want, bound, "score")
    assert torch.equal(got[:, 1:], res[:, :-1])
    # zeros exactly at each row's first real token and at masked slots
    zero = torch.zeros((2, 12), dtype=torch.bool)
    zero[:, 0] = True
    if padded:
        zero[0, :5] = True
    assert torch.equal((got == 0).cpu(), zero)
    # the decoder stands where prefill leaves it
    ref = _decoder("gemm", 2)
    ref.prefill(ids, attention_mask=mask)
    assert dec.positions == ref.positions and dec.position == ref.position and dec.tail is None
    assert dec.positions == ([8, 12] if padded else None)
    tok = torch.tensor([[5], [9]]).cuda()
    assert torch.equal(dec.step(tok), ref.step(tok))
    # perplexity, as the docstring shows it
    n_scored = int((~zero).sum())
    ppl = float(torch.exp(-got.sum() / n_scored))
    assert 1.0 < ppl < 64.0 ** 2


def test_score_equals_token_logprobs_of_prefill_on_one_row():
    from autoawq_amd import ops

    ids = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"]).cuda()[:1, :12]
    got = _decoder("gemm", 1).score(ids)
    logits = _decoder("gemm", 1).prefill(ids)
    want = ops.token_logprobs(logits[0, :-1], ids[0, 1:])
    assert torch.equal(got[0, 1:], want)


def test_fuse_mixtral_model():
    """the kernel sees only logits: the small Mixtral model of tests/test_mixtral.py, greedy and sampled"""
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    lm = fuse_mixtral(test_mixtral.build().cuda(), max_seq_len=48)
    dec = GraphedDecoder(lm, batch=2, buckets=(12, 24))
    ids = torch.randint(0, test_mixtral.V, (2, 6), generator=torch.Generator().manual_seed(9)).cuda()
    for cfg in ({}, {"do_sample": True, "temperature": 0.8, "top_k": 12, "seed": 5}):
        plain = dec.generate(ids, max_new_tokens=8, **cfg)
        out = dec.generate(ids, max_new_tokens=8, logprobs=True, **cfg)
        assert torch.equal(out, plain)
        new = out[:, 6:]
        _assert_values(dec.last_logprobs, _hand_logits(dec, ids, new), new, [8, 8], f"mixtral {sorted(cfg)}")
