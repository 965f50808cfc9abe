"""GraphedDecoder.generate end to end on the committed tiny-Llama checkpoints (MI355X): greedy equals the hand loop of
dec.step + torch.argmax; sampling equals a hand loop that feeds dec.step the restatement's tokens (tests/sampling_ref.py)."""
import numpy as np
import pytest
import torch

import sampling_ref as ref
from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
VERSIONS = ["gemm", "gemv", "gemv_fast"]


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


def _hand_loop(dec, prompt, n, pick):
    logits = dec.prefill(prompt)
    toks = []
    for i in range(n):
        tok = pick(logits[:, -1].float().cpu().numpy(), i + 1)
        toks.append(tok)
        if i + 1 < n:
            logits = dec.step(torch.tensor(tok, device="cuda").view(-1, 1))
    return torch.tensor(toks).T


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("batch", [1, 2])
def test_greedy_generate_equals_step_argmax_loop(version, batch):
    dec = _decoder(version, batch)
    prompt = _prompt(batch)
    out = dec.generate(prompt, max_new_tokens=10)
    assert out.shape == (batch, 16) and out.dtype == torch.int64
    assert torch.equal(out[:, :6].cpu(), prompt.cpu())
    hand = _hand_loop(dec, prompt, 10, lambda lg, t: np.argmax(lg, -1).tolist())
    assert torch.equal(out[:, 6:].cpu(), hand)
    assert sorted(dec.graphs) == [12, 24] and sorted(dec.gen_graphs) == [(12, True), (24, True)]


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("batch", [1, 2])
def test_sampled_generate_equals_restatement_loop(version, batch):
    cfg = {"temperature": 0.9, "top_k": 20, "top_p": 0.9}
    dec = _decoder(version, batch)
    prompt = _prompt(batch)
    out = dec.generate(prompt, max_new_tokens=10, do_sample=True, seed=11, **cfg).cpu()

    def pick(lg, t):  # the generated token where the restatement's margin leaves room, the restatement's token otherwise
        toks = []
        for r in range(lg.shape[0]):
            want, keep, s = ref.choose(lg[r].astype(np.float16), do_sample=True, seed=11, t=t, row=r, **cfg)
            got = int(out[r, 5 + t])
            assert keep[got] and abs(s[got] - s[want]) <= 1e-4 * max(1.0, abs(s[want])), (t, r, got, want)
            toks.append(got)
        return toks

    _hand_loop(dec, prompt, 10, pick)
    again = dec.generate(prompt, max_new_tokens=10, do_sample=True, seed=11, **cfg).cpu()
    assert torch.equal(out, again)
    other = dec.generate(prompt, max_new_tokens=10, do_sample=True, seed=12, **cfg).cpu()
    assert not torch.equal(out, other)


def test_window_roll_keeps_drawing_fresh_numbers():
    """max_seq_len 16: the run rolls the cache window (position resets) while the sampler's counter t keeps counting tokens.
    Every draw, before and after the roll, equals the restatement's draw at counter t on the logits a hand loop of dec.step
    (which rolls the same way) produces."""
    cfg = {"temperature": 1.5, "top_k": 0, "top_p": 1.0}
    dec = _decoder("gemv", 1, max_seq_len=16)
    prompt = _prompt(1)
    out = dec.generate(prompt, max_new_tokens=30, do_sample=True, seed=4, **cfg).cpu()
    assert out.shape == (1, 36)
    assert int(dec._gen["t"].item()) == 31   # t is the token index, not the position (which rolled)
    assert dec.position < 16
    seen_roll = []

    def pick(lg, t):
        want, keep, s = ref.choose(lg[0].astype(np.float16), do_sample=True, seed=4, t=t, row=0, **cfg)
        got = int(out[0, 5 + t])
        assert keep[got] and abs(s[got] - s[want]) <= 1e-4 * max(1.0, abs(s[want])), (t, got, want)
        seen_roll.append(dec.position)
        return [got]

    _hand_loop(dec, prompt, 30, pick)
    assert min(seen_roll[1:]) < max(seen_roll)   # the hand loop's positions went back: the draws span the roll
    assert len(set(out[0, 6:].tolist())) > 5


def test_eos_stops_early_and_pads():
    dec = _decoder("gemm", 2)
    prompt = _prompt(2)
    free = dec.generate(prompt, max_new_tokens=12).cpu()
    eos = int(free[0, 6 + 2])              # row 0 emits it as its third token
    out = dec.generate(prompt, max_new_tokens=12, eos_token_id=eos, pad_token_id=0, check_every=4).cpu()
    new = out[:, 6:]
    assert new[0, 2] == eos and (new[0, 3:] == 0).all()
    row1 = free[1, 6:].tolist()
    if eos in row1:                        # both rows finish: the run stops where the last one did
        assert new.shape[1] == max(3, row1.index(eos) + 1)
    else:
        assert new.shape[1] == 12 and new[1].tolist() == row1
