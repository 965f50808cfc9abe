"""GraphedDecoder with an attention_mask: prompts of different lengths in one batch, on the committed tiny-Llama checkpoints.

Logits at real positions equal transformers' LlamaForCausalLM (fp32, CPU, the mask and position_ids = cumsum(mask) - 1, the
dequantised weights of the loaded WQLinear modules).  Every row of a ragged run equals its prompt run through a uniform decoder
of the same batch size (the prompt repeated in every row, so the row keeps its Philox key), greedy and sampled, across a
per-row window roll and with EOS.  An all-ones mask is the unmasked call."""
import numpy as np
import pytest
import torch

import sampling_ref as ref
from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
VERSIONS = ["gemm", "gemv", "gemv_fast"]
TOL = 2e-2   # relative to the logit range: the checkpoint-logit tests' tolerance


def _decoder(version, batch, max_seq_len=32):
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    model, _ = load_quantized(skeleton(), ckpt(version), device="cuda")
    lm = fuse_llama(model, max_seq_len=max_seq_len)
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
    """prefill (with the mask) + one dec.step per column of toks [B, n - 1]: the logits [B, V] (float64) at every token index"""
    logits = dec.prefill(ids, attention_mask=mask)
    if mask is not None:
        last = mask.shape[1] - 1 - mask.flip(1).argmax(1)   # last real column of each row
        first = logits[torch.arange(ids.shape[0]), last]
    else:
        first = logits[:, -1]
    out = [first.double().cpu().numpy()]
    for i in range(toks.shape[1]):
        out.append(dec.step(toks[:, i:i + 1].cuda())[:, 0].double().cpu().numpy())
    return out


def _transformers_model(version):
    """fp32 LlamaForCausalLM on the CPU with the loaded checkpoint's weights, the int4 Linears dequantised by running them on
    the identity (exactly the fp16 weights the kernels multiply with)."""
    from autoawq_amd.checkpoint import load_quantized

    qm, _ = load_quantized(skeleton(), ckpt(version), device="cuda")
    hf = skeleton().float()
    hf.config._attn_implementation = "eager"
    sd = {k: v.float().cpu() for k, v in qm.state_dict().items() if k in hf.state_dict()}
    hf.load_state_dict(sd, strict=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
             "mlp.down_proj"]
    with torch.no_grad():
        for name in names:
            mod, dst = qm.model.layers[0].get_submodule(name), hf.model.layers[0].get_submodule(name)
            eye = torch.eye(mod.in_features, dtype=torch.float16, device="cuda")[None]
            dst.weight.copy_(mod(eye)[0].float().cpu().T)
    return hf.eval()


def _hf_logits(hf, ids, mask):
    pos = (mask.cumsum(1) - 1).clamp(min=0)
    with torch.no_grad():
        return hf(input_ids=ids.cpu(), attention_mask=mask.cpu(), position_ids=pos.cpu()).logits.double().numpy()


@pytest.mark.parametrize("version", VERSIONS)
def test_ragged_logits_match_transformers(version):
    lengths = [2, 6, 11]
    ids, mask = _left_padded(_prompts(lengths))
    dec = _decoder(version, 3)
    hf = _transformers_model(version)
    pre = dec.prefill(ids, attention_mask=mask).double().cpu().numpy()
    assert dec.positions == lengths and dec.graphs == {}
    steps = []
    tok = torch.from_numpy(pre[:, -1].argmax(-1)).view(-1, 1)
    toks = [tok]
    for _ in range(5):   # positions 2 .. 6, 6 .. 10, 11 .. 15: the last row crosses the 12-row bucket
        steps.append(dec.step(tok.cuda())[:, 0].double().cpu().numpy())
        tok = torch.from_numpy(steps[-1].argmax(-1)).view(-1, 1)
        toks.append(tok)
    assert dec.positions == [n + 5 for n in lengths] and sorted(dec.row_graphs) == [12, 24] and dec.graphs == {}
    full_ids = torch.cat([ids.cpu(), torch.cat(toks[:5], 1)], 1)
    full_mask = torch.cat([mask.cpu(), torch.ones((3, 5), dtype=torch.int64)], 1)
    want = _hf_logits(hf, full_ids, full_mask)
    S = ids.shape[1]
    rng = np.abs(want).max()
    real = mask.cpu().numpy().astype(bool)
    assert np.abs(pre[real] - want[:, :S][real]).max() <= TOL * rng
    for k, got in enumerate(steps):
        assert np.abs(got - want[:, S + k]).max() <= TOL * rng, k


def _check_row(got_tok, lg_alone, lg_ragged, t, row, sample_cfg):
    """got_tok (the ragged run's token at index t) against the prompt alone: greedy -- equal to the argmax wherever the top-2
    margin is above the tolerance; sampled -- the restatement's draw on the logits alone, with test_gpu_generate's margin rule
    widened by how far the two runs' logits are apart (the same Gumbel term is added to both)."""
    rng = np.abs(lg_alone).max()
    if sample_cfg is None:
        top = np.sort(lg_alone)[-2:]
        if top[1] - top[0] > TOL * rng:
            assert got_tok == int(np.argmax(lg_alone)), (t, row)
        return
    want, keep, s = ref.choose(lg_alone.astype(np.float16), do_sample=True, t=t, row=row, **sample_cfg)
    drift = np.abs(lg_alone - lg_ragged).max() / sample_cfg["temperature"]
    assert keep[got_tok] or drift > 0, (t, row)
    assert np.isfinite(s[got_tok]) and abs(s[got_tok] - s[want]) <= 1e-4 * max(1.0, abs(s[want])) + 2 * drift, (t, row, got_tok, want)


def _each_row_alone(version, lengths, n, sample_cfg, max_seq_len=32):
    B = len(lengths)
    prompts = _prompts(lengths)
    ids, mask = _left_padded(prompts)
    dec = _decoder(version, B, max_seq_len)
    kw = {} if sample_cfg is None else dict(do_sample=True, **sample_cfg)
    out = dec.generate(ids, max_new_tokens=n, attention_mask=mask, **kw).cpu()
    assert out.shape == (B, ids.shape[1] + n) and torch.equal(out[:, :ids.shape[1]], ids.cpu())
    assert dec.graphs == {} and dec.gen_graphs == {} and dec.row_gen_graphs
    new = out[:, ids.shape[1]:]
    ragged = _hand_loop(dec, ids, mask, new[:, :-1])
    for b, p in enumerate(prompts):
        alone_dec = _decoder(version, B, max_seq_len)
        alone = _hand_loop(alone_dec, p.view(1, -1).repeat(B, 1).cuda(), None, new[b:b + 1, :-1].repeat(B, 1))
        for t in range(n):
            _check_row(int(new[b, t]), alone[t][b], ragged[t][b], t + 1, b, sample_cfg)
    return dec, out


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("sampled", [False, True])
def test_each_ragged_row_equals_its_prompt_alone(version, sampled):
    cfg = {"temperature": 0.9, "top_k": 20, "top_p": 0.9, "seed": 11} if sampled else None
    _each_row_alone(version, [2, 6, 11], 10, cfg)


@pytest.mark.parametrize("sampled", [False, True])
def test_per_row_window_roll(sampled):
    """max_seq_len 16: the 11-token row runs past the window after 5 tokens and rolls on its own; the 2-token row never does.
    Both still equal their prompts run alone (which roll at the same tokens)."""
    cfg = {"temperature": 1.5, "top_k": 0, "top_p": 1.0, "seed": 4} if sampled else None
    dec, out = _each_row_alone("gemv", [2, 11], 12, cfg, max_seq_len=16)
    assert out.shape == (2, 23)
    # after the hand loop's 11 steps: row 0 at 2 + 11; row 1 reached 16, forgot all of it (the reference's roll), then 6 more
    assert dec.positions == [13, 6]


def test_ragged_eos_stops_early_and_pads():
    lengths = [3, 6]
    ids, mask = _left_padded(_prompts(lengths))
    dec = _decoder("gemm", 2)
    S = ids.shape[1]
    free = dec.generate(ids, max_new_tokens=12, attention_mask=mask).cpu()
    eos = int(free[0, S + 2])               # row 0 emits it as its third token
    out = dec.generate(ids, max_new_tokens=12, eos_token_id=eos, pad_token_id=0, check_every=4, attention_mask=mask).cpu()
    new = out[:, S:]
    assert new[0, 2] == eos and (new[0, 3:] == 0).all()
    row1 = free[1, S:].tolist()
    if eos in row1:
        assert new.shape[1] == max(3, row1.index(eos) + 1)
    else:
        assert new.shape[1] == 12 and new[1].tolist() == row1


@pytest.mark.parametrize("version", VERSIONS)
def test_all_ones_mask_is_the_unmasked_call(version):
    ids = torch.from_numpy(golden("tiny_llama_awq_gemm_outputs")["input_ids"][:, :6].copy()).cuda()
    dec = _decoder(version, 2)
    plain = dec.generate(ids, max_new_tokens=8).cpu()
    pre = dec.prefill(ids).clone()
    ones = torch.ones_like(ids)
    masked = dec.generate(ids, max_new_tokens=8, attention_mask=ones).cpu()
    assert torch.equal(plain, masked)
    assert torch.equal(pre, dec.prefill(ids, attention_mask=ones))
    sampled = dict(do_sample=True, temperature=0.9, top_k=20, seed=3)
    assert torch.equal(dec.generate(ids, max_new_tokens=8, **sampled).cpu(),
                       dec.generate(ids, max_new_tokens=8, attention_mask=ones, **sampled).cpu())
    assert dec.row_graphs == {} and dec.row_gen_graphs == {} and dec.positions is None
