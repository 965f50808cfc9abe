"""GraphedDecoder.generate with repetition_penalty and min_new_tokens, end to end on the committed tiny-Llama checkpoints
(MI355X).  The oracle is a hand loop: dec.prefill / dec.step for the logits, then the restatement sampling_ref.choose(
penalty_ref.process(...)) fed a numpy history of the prompt as passed (pad columns included) and the tokens so far.  Greedy is
exact; a sampled token is checked as in tests/test_gpu_generate.py."""
import numpy as np
import pytest
import torch

import penalty_ref as pref
import sampling_ref as ref
from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
VERSIONS = ["gemm", "gemv", "gemv_fast"]
SAMPLED = {"temperature": 0.9, "top_k": 20, "top_p": 0.9}


def _decoder(version, batch, max_seq_len=32):
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    model, _ = load_quantized(skeleton(), ckpt(version), device="cuda")
    lm = fuse_llama(model, max_seq_len=max_seq_len)
    return GraphedDecoder(lm, batch=batch, buckets=(12, 24))


def _prompt(batch):
    ids = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"]).cuda()
    return ids[:batch, :6] if batch <= ids.shape[0] else ids[:1, :6].repeat(batch, 1)


def _check(out, ids, dec, n, *, p, min_new, eos=(), sampled=None, seed=0, mask=None, pad=None):
    """Replay generate's run as a hand loop and check every token of `out` [B, S + n'] against the restatement."""
    B, S = ids.shape
    new = out[:, S:].numpy()
    logits = dec.prefill(ids, attention_mask=mask)
    if mask is not None:
        last = mask.shape[1] - 1 - mask.flip(1).argmax(1)
        lg = logits[torch.arange(B), last]
    else:
        lg = logits[:, -1]
    seen = [list(r) for r in ids.cpu().numpy()]
    finished = [False] * B
    for i in range(new.shape[1]):
        t = i + 1
        x = lg.float().cpu().numpy().astype(np.float16)
        for r in range(B):
            got = int(new[r, i])
            if finished[r]:
                want = eos[0] if pad is None else pad
            else:
                v = pref.process(x[r], pref.seen_mask(pref.bitmap([seen[r]], x.shape[1])[0], x.shape[1]), t=t,
                                 repetition_penalty=p, min_new_tokens=min_new, eos_ids=eos)
                if sampled is None:
                    want = ref.choose(v, do_sample=False)[0]
                else:
                    want, keep, s = ref.choose(v, do_sample=True, seed=seed, t=t, row=r, **sampled)
                    assert keep[got] and abs(s[got] - s[want]) <= 1e-4 * max(1.0, abs(s[want])), (t, r, got, want)
                    want = got
            assert got == want, (t, r, got, want)
            if got in eos:
                finished[r] = True
            seen[r].append(got)
        if i + 1 < new.shape[1]:
            lg = dec.step(torch.from_numpy(new[:, i].copy()).cuda().view(-1, 1))[:, 0]


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("batch", [1, 2])
def test_greedy_and_sampled_generate_equal_hand_loop(version, batch):
    dec = _decoder(version, batch)
    prompt = _prompt(batch)
    free = dec.generate(prompt, max_new_tokens=10).cpu()
    eos = [int(free[0, 6 + 1])]
    out = dec.generate(prompt, max_new_tokens=10, repetition_penalty=1.3, min_new_tokens=4, eos_token_id=eos).cpu()
    assert torch.equal(out[:, :6], prompt.cpu())
    _check(out, prompt, dec, 10, p=1.3, min_new=4, eos=eos)
    assert not torch.equal(out[:, 6:], free[:, 6:out.shape[1]])     # the processors changed the greedy run
    out = dec.generate(prompt, max_new_tokens=10, do_sample=True, seed=11, repetition_penalty=1.3, min_new_tokens=4,
                       eos_token_id=eos, **SAMPLED).cpu()
    _check(out, prompt, dec, 10, p=1.3, min_new=4, eos=eos, sampled=SAMPLED, seed=11)
    assert dec.proc_gen_graphs and sorted(dec.gen_graphs) == [(12, True), (24, True)]


def test_left_padded_batch_penalises_its_pads():
    """A left-padded attention_mask batch; the pad id is in every padded row's history, as in transformers' input_ids."""
    dec = _decoder("gemv", 2)
    ids = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"]).cuda()
    pad_id = 5
    batch = torch.full((2, 7), pad_id, dtype=torch.int64, device="cuda")
    mask = torch.zeros((2, 7), dtype=torch.int64, device="cuda")
    batch[0, :] = ids[0, :7]
    mask[0, :] = 1
    batch[1, 3:] = ids[1 % ids.shape[0], :4]
    mask[1, 3:] = 1
    for sampled in (None, SAMPLED):
        kw = {} if sampled is None else dict(do_sample=True, seed=3, **sampled)
        out = dec.generate(batch, max_new_tokens=8, attention_mask=mask, repetition_penalty=1.3, **kw).cpu()
        _check(out, batch, dec, 8, p=1.3, min_new=0, sampled=sampled, seed=3, mask=mask)
    assert dec.row_proc_gen_graphs and not dec.row_gen_graphs


@pytest.mark.parametrize("sampled", [False, True])
def test_penalty_survives_the_window_roll(sampled):
    """max_seq_len 32, 6 prompt tokens and 30 new: the cache window rolls, and the history (like transformers' input_ids) still
    holds the tokens whose cache rows were rolled away."""
    dec = _decoder("gemv", 1, max_seq_len=32)
    prompt = _prompt(1)
    kw = {} if not sampled else dict(do_sample=True, seed=4, temperature=1.2)
    out = dec.generate(prompt, max_new_tokens=30, repetition_penalty=1.3, **kw).cpu()
    assert out.shape == (1, 36) and dec.position < 32
    _check(out, prompt, dec, 30, p=1.3, min_new=0, sampled=None if not sampled else {"temperature": 1.2}, seed=4)
    hist = pref.seen_mask(dec._gen["history"][0].cpu().numpy(), dec._gen["vocab"])
    assert set(np.flatnonzero(hist).tolist()) == set(out[0].tolist())


def test_min_new_tokens_holds_eos_back():
    """eos_token_id = the token greedy emits second: with min_new_tokens = 5 no row stops before token 6."""
    dec = _decoder("gemm", 2)
    prompt = _prompt(2)
    free = dec.generate(prompt, max_new_tokens=12).cpu()
    eos = int(free[0, 6 + 1])
    early = dec.generate(prompt, max_new_tokens=12, eos_token_id=eos, pad_token_id=0).cpu()
    assert early[0, 6 + 1] == eos and (early[0, 6 + 2:] == 0).all()
    out = dec.generate(prompt, max_new_tokens=12, eos_token_id=eos, pad_token_id=0, min_new_tokens=5, check_every=4).cpu()
    new = out[:, 6:]
    assert new.shape[1] >= 6 and (new[:, :5] != eos).all()
    _check(out, prompt, dec, 12, p=1.0, min_new=5, eos=[eos], pad=0)


def test_defaults_take_todays_graphs():
    dec = _decoder("gemv", 2)
    prompt = _prompt(2)
    a = dec.generate(prompt, max_new_tokens=10).cpu()
    b = dec.generate(prompt, max_new_tokens=10, repetition_penalty=1.0, min_new_tokens=0).cpu()
    assert torch.equal(a, b)
    assert sorted(dec.gen_graphs) == [(12, True), (24, True)]
    assert dec.proc_gen_graphs == {} and dec.row_proc_gen_graphs == {}
    dec.generate(prompt, max_new_tokens=10, repetition_penalty=1.2)
    assert sorted(dec.gen_graphs) == [(12, True), (24, True)] and sorted(dec.proc_gen_graphs) == [(12, True), (24, True)]
    with pytest.raises(ValueError):
        dec.generate(prompt, max_new_tokens=4, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        dec.generate(prompt, max_new_tokens=4, min_new_tokens=-1)
