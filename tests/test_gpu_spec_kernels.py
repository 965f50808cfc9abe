"""awq_spec_accept and awq_ngram_draft (csrc/spec.hip) equal tests/spec_ref.py exactly on randomised states: no match, a match at
index 0, a match whose continuation runs into the end, every accepted length 0 .. T - 1, EOS inside the accepted run, the budget
ending inside it, finished rows untouched, batch sizes that are a multiple of nothing."""
import numpy as np
import pytest
import torch

import spec_ref

pytestmark = pytest.mark.gpu


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


@pytest.mark.parametrize("T", [2, 3, 5, 8])
@pytest.mark.parametrize("ngram_max", [1, 2, 3])
def test_ngram_draft_equals_reference(T, ngram_max):
    from autoawq_amd import ops

    rng = np.random.default_rng(100 * T + ngram_max)
    cap = 700
    fixed = [[7], [1, 2, 3, 4], [1, 2, 3, 9, 1, 2, 3], [5, 1, 2, 8, 1, 2], [1, 2, 7, 1, 2, 8, 1, 2], [3, 1, 9, 2, 1], [4, 4, 4]]
    rows = list(fixed)
    for n in (2, 3, 17, 255, 256, 257, 300, 513, 700):       # around the block's 256-thread stride; small vocabularies repeat
        rows.append(list(rng.integers(0, 3, size=n)))
        rows.append(list(rng.integers(0, 50, size=n)))        # mostly no match
        r = list(rng.integers(0, 1000, size=n))
        if n > 8:
            r[-3:] = r[:3]                                     # a match at index 0 only
        rows.append(r)
    B = len(rows)                                              # 34: a multiple of nothing the kernels care about
    hist = np.full((B, cap), -5, dtype=np.int32)
    n_hist = np.zeros(B, dtype=np.int32)
    for b, r in enumerate(rows):
        hist[b, :len(r)] = r
        n_hist[b] = len(r)
    params = ops.spec_params(max_new_tokens=10, ngram_max=ngram_max).cuda()
    tok = torch.full((B, T), -1, dtype=torch.int64, device="cuda")
    ops.ngram_draft(params, tok, _dev(hist, torch.int32), _dev(n_hist, torch.int32))
    got = tok.cpu().numpy()
    for b, r in enumerate(rows):
        assert got[b].tolist() == spec_ref.draft(r, T, ngram_max), (b, len(r))


@pytest.mark.parametrize("T", [2, 3, 5, 8])
def test_spec_accept_equals_reference(T):
    from autoawq_amd import ops

    rng = np.random.default_rng(T)
    B, ring_cap, hist_cap, max_new = 37, 40, 90, 30
    eos = (3, 11)
    tok = rng.integers(0, 20, size=(B, T)).astype(np.int64)
    pred = rng.integers(0, 20, size=(B, T)).astype(np.int64)
    for b in range(B):                                         # every accepted length 0 .. T - 1, several times over
        a = b % T
        pred[b, :a] = tok[b, 1:a + 1]
        if a < T - 1 and pred[b, a] == tok[b, a + 1]:
            pred[b, a] = (pred[b, a] + 1) % 20
    pred[5, :] = tok[5, 0] = 7                                 # a filler run: drafts equal to the argmax are accepted
    tok[5, :] = 7
    state = {"hist": rng.integers(0, 20, size=(B, hist_cap)).astype(np.int32),
             "n_hist": rng.integers(1, 50, size=B).astype(np.int32),
             "cnt": rng.integers(1, max_new, size=B).astype(np.int32),
             "ring": rng.integers(0, 20, size=(B, ring_cap)).astype(np.int32),
             "finished": (rng.random(B) < 0.2).astype(np.int32),
             "pos_rows": rng.integers(0, 100, size=B).astype(np.int32),
             "len_rows": rng.integers(0, 100, size=B).astype(np.int32)}
    state["cnt"][::7] = max_new - 2                            # the budget ends inside an accepted run
    state["finished"][[0, 1, 2, 3, 4, 5, 6, 7]] = 0
    bad = np.zeros(B, dtype=bool)
    bad[[9, 20]] = True                                        # a status bit in one of the row's slots
    status = np.zeros((B * T + 31) // 32, dtype=np.int64)
    for b, j in ((9, 0), (20, T - 1)):
        status[(b * T + j) // 32] |= 1 << ((b * T + j) % 32)
    status = status.astype(np.uint32).view(np.int32)
    dev = {k: _dev(v, torch.int32) for k, v in state.items()}
    params = ops.spec_params(eos_ids=eos, max_new_tokens=max_new, ngram_max=2).cuda()
    tok_d = _dev(tok, torch.int64)
    steps = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    ops.spec_accept(params, tok_d, _dev(pred.reshape(-1), torch.int64), dev["hist"], dev["n_hist"], dev["cnt"], dev["ring"],
                    dev["finished"], dev["pos_rows"], dev["len_rows"], status=_dev(status, torch.int32), steps=steps)
    before = {k: v.copy() for k, v in state.items()}
    spec_ref.accept_state(state, tok, pred, {"max_new_tokens": max_new, "eos": eos}, status_bad=bad)
    for name, want in state.items():
        assert np.array_equal(dev[name].cpu().numpy(), want), name
    assert np.array_equal(tok_d.cpu().numpy(), tok)
    moved = state["cnt"] - before["cnt"]
    was_finished = before["finished"] == 1
    assert (moved[was_finished] == 0).all() and (moved[~was_finished & ~bad] >= 1).all()
    assert set(moved[~was_finished & ~bad].tolist()) >= set(range(1, min(T, 3) + 1))     # short and long runs both occurred
    assert (state["cnt"] <= max_new).all()
    assert np.array_equal(steps.cpu().numpy(), 5 + (moved > 0))


def test_spec_refusals():
    from autoawq_amd import _lib, ops

    params = ops.spec_params().cuda()
    hist = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    n = torch.ones(1, dtype=torch.int32, device="cuda")
    for T in (1, 9):
        with pytest.raises(_lib.AwqHipError) as e:
            ops.ngram_draft(params, torch.zeros((1, T), dtype=torch.int64, device="cuda"), hist, n)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.spec_params(ngram_max=0)
