"""GraphedDecoder with kv_cache_dtype="fp8" end to end, against the fp16 decoder whose appended rows are passed through the
format's quantize -> dequantize (the unfused append, FUSE_ROPE_INTO_ATTENTION = False): prefill and 24 greedy steps on the
tiny-Llama checkpoints (all three layouts), with left padding, across a window roll, and on the small Mixtral model."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_checkpoint import ckpt, skeleton

pytestmark = pytest.mark.gpu
VERSIONS = ["gemm", "gemv", "gemv_fast"]
TOL = 2e-2   # relative to the logit range: the checkpoint-logit tests' tolerance


def test_reference_quantizer_on_the_gpu_matches_the_restatement():
    """The reference below fake-quantizes on the device with the torch form of the format (a captured graph replays it; the
    numpy restatement cannot run there): it agrees with tests/kv8_ref.py bit for bit on CUDA tensors too."""
    from test_kv8_cpu import _varied_rows
    import kv8_ref as ref
    from autoawq_amd.modules.fused.cache import dequantize_rows_fp8, quantize_rows_fp8

    x = _varied_rows(seed=11)
    c, s = quantize_rows_fp8(torch.from_numpy(x).cuda())
    rc, rs = ref.quantize(x)
    gs = s.cpu().numpy()
    bad_s = ~((gs == rs) | (np.isnan(gs) & np.isnan(rs)))
    bad_c = (c.cpu().numpy() != rc).any(-1)
    assert not bad_s.any() and not bad_c.any(), (int(bad_s.sum()), int(bad_c.sum()), np.nonzero(bad_c)[0][:5],
                                                 np.abs(x[bad_c][:3].astype(np.float32)).max(-1) if bad_c.any() else None)
    back = dequantize_rows_fp8(c, s).cpu().numpy()
    assert np.array_equal(back, ref.dequantize_fp16(rc, rs), equal_nan=True)


@pytest.fixture
def fake_quant_reference(monkeypatch):
    """fp16 decoders built inside this fixture's scope append fake-quantized rows: every append re-quantizes the whole cache
    (the format is idempotent on already quantized rows, so this equals quantizing the new rows only) with torch ops, which a
    captured graph replays."""
    from autoawq_amd import ops
    from autoawq_amd.modules.fused.attn import QuantAttentionFused
    from autoawq_amd.modules.fused.cache import dequantize_rows_fp8, quantize_rows_fp8

    real = ops.rope_kv_append

    def append(qkv, k_cache, v_cache, *a, **kw):
        q = real(qkv, k_cache, v_cache, *a, **kw)
        if k_cache.dtype == torch.float16:
            for c in (k_cache, v_cache):
                c.copy_(dequantize_rows_fp8(*quantize_rows_fp8(c)))
        return q

    monkeypatch.setattr(ops, "rope_kv_append", append)
    monkeypatch.setattr(QuantAttentionFused, "FUSE_ROPE_INTO_ATTENTION", False)


def _lm(version, kv, max_seq_len):
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama

    model, _ = load_quantized(skeleton(), ckpt(version), device="cuda")
    return fuse_llama(model, max_seq_len=max_seq_len, kv_cache_dtype=kv) if kv else fuse_llama(model, max_seq_len=max_seq_len)


def _run(lm, ids, mask, steps):
    """prefill + `steps` greedy tokens: (list of float64 logits [B, V] per step, generated ids)"""
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    dec = GraphedDecoder(lm, batch=ids.shape[0], buckets=(12, 24))
    logits = dec.prefill(ids, attention_mask=mask)
    if mask is not None:
        last = mask.shape[1] - 1 - mask.flip(1).argmax(1)
        cur = logits[torch.arange(ids.shape[0]), last]
    else:
        cur = logits[:, -1]
    got = [cur.double().cpu().numpy()]
    toks = []
    for _ in range(steps):
        nxt = cur.argmax(-1, keepdim=True)
        toks.append(nxt)
        cur = dec.step(nxt)[:, 0]
        got.append(cur.double().cpu().numpy())
    return got, torch.cat(toks, 1) if toks else None


def _close(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        rng = y.max() - y.min()
        assert np.abs(x - y).max() <= TOL * rng, (i, np.abs(x - y).max(), rng)


def _ids(B, S):
    ids = golden("tiny_llama_awq_gemm_outputs")["input_ids"]
    return torch.from_numpy(np.stack([ids[b % ids.shape[0], :S] for b in range(B)])).long().cuda()


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("case", ["plain", "left_padded", "roll"])
def test_fp8_decoder_vs_fake_quant_fp16(fake_quant_reference, version, case):
    B, S, steps = 2, 8, 24
    max_seq_len = 20 if case == "roll" else 64  # 8 + 24 tokens run past a 20-row window
    ids = _ids(B, S)
    mask = None
    if case == "left_padded":
        mask = torch.ones_like(ids)
        mask[1, :3] = 0
        ids[1, :3] = 0
    lm8 = _lm(version, "fp8", max_seq_len)
    assert lm8.kv_cache_dtype == "fp8" and lm8.model.blocks[0].attn.cache.k.dtype == torch.uint8
    got, toks = _run(lm8, ids, mask, steps)
    want, _ = _run(_lm(version, "fp16", max_seq_len), ids, mask, 0)
    _close(got[:1], want)
    # teacher-force the reference on the fp8 run's tokens
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    ref = GraphedDecoder(_lm(version, "fp16", max_seq_len), batch=B, buckets=(12, 24))
    ref.prefill(ids, attention_mask=mask)
    want = [want[0]] + [ref.step(toks[:, i:i + 1].contiguous())[:, 0].double().cpu().numpy() for i in range(steps)]
    _close(got, want)
    if case == "plain":  # the generation graphs (step + on-device sampler) over the fp8 cache: the hand loop's greedy tokens
        gen = GraphedDecoder(_lm(version, "fp8", max_seq_len), batch=B, buckets=(12, 24))
        out = gen.generate(ids, max_new_tokens=steps, do_sample=False)
        assert torch.equal(out[:, S:].cpu(), toks.cpu())


def test_default_is_bitwise_unchanged():
    ids = _ids(2, 8)
    a, _ = _run(_lm("gemv", None, 64), ids, None, 6)
    b, _ = _run(_lm("gemv", "fp16", 64), ids, None, 6)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_mixtral_fp8(fake_quant_reference):
    import test_mixtral
    from autoawq_amd.fuser import fuse_mixtral

    def lm(kv):
        m = test_mixtral.build().cuda()
        return fuse_mixtral(m, max_seq_len=48, kv_cache_dtype=kv)

    ids = torch.randint(0, test_mixtral.V, (2, 6), generator=torch.Generator().manual_seed(9)).cuda()
    lm8 = lm("fp8")
    assert lm8.kv_cache_dtype == "fp8"
    got, toks = _run(lm8, ids, None, 8)
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    ref = GraphedDecoder(lm("fp16"), batch=2, buckets=(12, 24))
    want = [ref.prefill(ids)[:, -1].double().cpu().numpy()]
    want += [ref.step(toks[:, i:i + 1].contiguous())[:, 0].double().cpu().numpy() for i in range(8)]
    _close(got, want)
