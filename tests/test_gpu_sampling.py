"""csrc/sample.hip against the fp64 restatement of tests/sampling_ref.py (MI355X).  Greedy is exact; a sampled token must be
kept by the restatement and its fp64 Gumbel score within 1e-4 (relative) of the restatement's best, and equal to the
restatement's token wherever the restatement's margin exceeds that."""
import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import _lib, ops as o

    _lib.lib()
    return o


def _logits(B, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, V), generator=g) * scale).half()


def _check_sampled(row_logits, tok, cfg, t, row, seed):
    want, keep, s = ref.choose(row_logits, do_sample=True, seed=seed, t=t, row=row, **cfg)
    assert keep[tok], (tok, want)
    best = s[want]
    assert abs(s[tok] - best) <= TOL * max(1.0, abs(best)), (tok, want, s[tok], best)
    runner_up = np.sort(s[np.isfinite(s)])[-2] if np.isfinite(s).sum() > 1 else -np.inf
    if best - runner_up > 2 * TOL * max(1.0, abs(best)):
        assert tok == want
    return want


@pytest.mark.parametrize("V", [64, 1000, 32000, 128256, 152064])
@pytest.mark.parametrize("B", [1, 4, 16])
def test_greedy_is_argmax(ops, B, V):
    x = _logits(B, V, B * 7 + V)
    x[0, V // 3] = x[0].max() + 1
    x[0, V // 2] = x[0, V // 3]          # tie: the lower index wins
    if B > 1:
        x[1] = 0.5                       # all equal: index 0
        x[1, V - 1] = -0.0
    out = ops.sample_tokens(x.cuda(), do_sample=False)
    assert out.cpu().tolist() == torch.argmax(x.float(), -1).tolist()
    assert out[0].item() == V // 3


@pytest.mark.parametrize("V", [64, 1000, 32000, 128256, 152064])
@pytest.mark.parametrize("B", [1, 4, 16])
def test_sampling_matches_restatement(ops, B, V):
    x = _logits(B, V, B * 13 + V)
    for cfg in ({"temperature": 0.7, "top_k": 50, "top_p": 0.9}, {"temperature": 1.0, "top_k": 0, "top_p": 1.0},
                {"temperature": 1.3, "top_k": 0, "top_p": 0.5}, {"temperature": 1.0, "top_k": min(V, 5000), "top_p": 1.0}):
        for t in (1, 7):
            out = ops.sample_tokens(x.cuda(), do_sample=True, seed=42, t=t, **cfg).cpu().numpy()
            for r in range(B):
                _check_sampled(x[r].numpy(), int(out[r]), cfg, t, r, 42)


def test_strided_last_position_view(ops):
    B, T, V = 4, 3, 1000
    x = _logits(B * T, V, 5).reshape(B, T, V)
    big = torch.full((B, T, V + 8), float("nan")).half()
    big[:, :, :V] = x
    xs = big.cuda()[:, :, :V]            # rows V + 8 elements apart, unaligned past row 0
    g = ops.sample_tokens(xs, do_sample=False).cpu()
    assert g.tolist() == torch.argmax(x[:, -1].float(), -1).tolist()
    cfg = {"temperature": 0.8, "top_k": 40, "top_p": 0.95}
    s = ops.sample_tokens(xs, do_sample=True, seed=3, t=2, **cfg).cpu().numpy()
    for r in range(B):
        _check_sampled(x[r, -1].numpy(), int(s[r]), cfg, 2, r, 3)


@pytest.mark.parametrize("V", [1000, 152064])
def test_top_k_one_and_tiny_top_p_are_argmax(ops, V):
    x = _logits(4, V, V + 1)
    want = torch.argmax(x.float(), -1).tolist()
    for t in range(1, 4):
        assert ops.sample_tokens(x.cuda(), do_sample=True, top_k=1, seed=t, t=t).cpu().tolist() == want
        assert ops.sample_tokens(x.cuda(), do_sample=True, top_p=1e-6, seed=t, t=t).cpu().tolist() == want


def test_ties_at_the_boundaries_kept_whole(ops):
    V = 64
    x = torch.full((1, V), -2.0).half()
    x[0, :4] = 3.0                        # four-way tie at the top-k = 2 boundary: all four kept
    seen = set()
    for t in range(1, 200):
        tok = int(ops.sample_tokens(x.cuda(), do_sample=True, top_k=2, seed=9, t=t)[0])
        seen.add(tok)
        assert ref.choose(x[0].numpy(), do_sample=True, top_k=2, seed=9, t=t)[0] == tok
    assert seen == {0, 1, 2, 3}


def test_neg_inf_never_chosen_nan_and_inf_rows_flagged(ops):
    from autoawq_amd import _lib

    V = 3000
    x = _logits(4, V, 77)
    x[:, ::2] = float("-inf")
    for t in range(1, 20):
        out = ops.sample_tokens(x.cuda(), do_sample=True, seed=1, t=t).cpu()
        assert (out % 2 == 1).all()
    y = x.clone()
    y[1, 5] = float("nan")
    y[2, 7] = float("inf")
    y[3] = float("-inf")
    for do_sample in (False, True):
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = ops.sample_tokens(y.cuda(), do_sample=do_sample, pad=-7, status=status).cpu()
        assert out[1:].tolist() == [-7, -7, -7] and out[0] != -7
        assert int(status.item()) == 0b1110
        with pytest.raises(_lib.AwqHipError):
            ops.sample_tokens(y.cuda(), do_sample=do_sample)


def test_frequencies_follow_the_distribution(ops):
    """4096 (t, row) draws at V = 16 against the restatement's probabilities: a chi-square bound (deterministic: fixed seed)."""
    V, B = 16, 16
    row = (torch.linspace(-2, 2, V) + torch.tensor([0.3 * (i % 3) for i in range(V)])).half()
    x = row.repeat(B, 1).cuda()
    for cfg in ({"temperature": 1.0, "top_k": 0, "top_p": 1.0}, {"temperature": 0.8, "top_k": 10, "top_p": 0.8}):
        counts = np.zeros(V)
        for t in range(1, 4096 // B + 1):
            out = ops.sample_tokens(x, do_sample=True, seed=2024, t=t, **cfg).cpu().numpy()
            np.add.at(counts, out, 1)
        p = ref.probabilities(row.numpy(), **cfg)
        assert counts[p == 0].sum() == 0
        e = 4096 * p[p > 0]
        chi2 = ((counts[p > 0] - e) ** 2 / e).sum()
        assert chi2 < 45.0, (chi2, counts, e)  # dof <= 15: p(chi2 > 45) ~ 1e-4


def test_bookkeeping_t_ring_eos_and_clean_workspace(ops):
    B, V, cap = 3, 1000, 8
    x = _logits(B, V, 11)
    xd = x.cuda()
    t = torch.ones(1, dtype=torch.int32, device="cuda")
    ring = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
    fin = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros((B, 1), dtype=torch.int64, device="cuda")
    greedy = torch.argmax(x.float(), -1)
    eos = [int(greedy[1]), 999999]
    for step in range(1, 6):
        do_sample = step % 2 == 0
        ops.sample_tokens(xd, do_sample=do_sample, seed=5, t=t, eos_ids=eos, pad=-1, out=out, ring=ring, finished=fin)
        assert int(t.item()) == step + 1
        ws = ops._sample_workspace(xd.device, ops.sample_workspace_bytes(B, V))
        assert int(ws.count_nonzero()) == 0, step
        got = ring[:, step - 1].cpu()
        assert out[:, 0].cpu().tolist() == got.tolist()
        assert got[1].item() == (eos[0] if step == 1 else -1)   # EOS latched after the first token, pad after it
        for r in (0, 2):
            if not do_sample:
                assert got[r].item() == greedy[r].item()
            else:
                _check_sampled(x[r].numpy(), int(got[r]), {"temperature": 1.0, "top_k": 0, "top_p": 1.0}, step, r, 5)
    assert fin.cpu().tolist() == [0, 1, 0]
    assert (ring[:, 5:] == -1).all()


def test_bad_row_pad_does_not_latch_finished(ops):
    """A NaN / +inf row emits pad and sets its status bit; pad defaults to the first EOS id, but a pad that was not sampled must
    not mark the row finished."""
    V = 1000
    x = _logits(3, V, 21)
    x[1, 3] = float("nan")
    xd = x.cuda()
    eos = int(torch.argmax(x[2].float()))
    for do_sample in (False, True):
        fin = torch.zeros(3, dtype=torch.int32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = ops.sample_tokens(xd, do_sample=do_sample, top_k=1, eos_ids=[eos], finished=fin, status=status).cpu()
        assert out[1].item() == eos and int(status.item()) == 0b10   # pad (= the EOS id) for the bad row
        assert fin.cpu().tolist() == [0, 0, 1]                       # only the row that SAMPLED the EOS id finished


def test_unsupported_shapes(ops):
    from autoawq_amd import _lib

    with pytest.raises(_lib.AwqHipError):
        ops.sample_tokens(torch.zeros((1025, 8), dtype=torch.float16, device="cuda"), do_sample=False)
