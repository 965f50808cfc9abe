"""The sampler's rows form (awq_sample_tokens_rows, csrc/sample.hip) on MI355X: row r of a launch with per-row parameters and
token indices against row r of the shared launch with that row's values (bit for bit) and against the fp64 restatement
tests/sampling_ref.py; uniform rows against the shared launch word for word; the per-row bookkeeping (ring slot, t, EOS and
budget latches, pads, status bits); min_new_tokens at per-row token indices; a captured launch replayed over parameters
rewritten in place.  B in {1, 3, 33} (33 crosses a status word), V in {1, 2047, 2049, 5000} (both sides of the 2048-element
chunk, several chunks).

The restatement draws in fp64 and the kernel in fp32: a sampled token is held to it as tests/test_gpu_sampling_penalty.py holds
one (inside the kept set, its score within TOL of the best, equal whenever the best leads by more than 2 TOL); the greedy token
and every comparison with the shared launch are exact."""
import numpy as np
import pytest
import torch

import penalty_ref as pref
import sampling_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
BS, VS = [1, 3, 33], [1, 2047, 2049, 5000]


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import _lib, ops as o

    _lib.lib()
    return o


def _logits(B, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, V), generator=g) * scale).half()


def _row_configs(B, V, seed):
    """per-row parameters: greedy and sampled rows, top_k / top_p on and off, different seeds and token indices"""
    rng = np.random.default_rng(seed)
    cfg = {"do_sample": [bool(r % 3) for r in range(B)] if B > 1 else [True],
           "temperature": [float(rng.choice([0.6, 1.0, 1.4])) for _ in range(B)],
           "top_k": [int(rng.choice([0, 1, 5, max(1, V // 3)])) if V > 1 else int(rng.integers(0, 2)) for _ in range(B)],
           "top_p": [float(rng.choice([1.0, 0.9, 0.5])) for _ in range(B)],
           "seed": [int(rng.integers(0, 2 ** 62)) for _ in range(B)]}
    t = [int(rng.integers(1, 40)) for _ in range(B)]
    return cfg, t


def _row(cfg, r):
    return {k: v[r] for k, v in cfg.items()}


def _check_ref(v, tok, c, t, row):
    if not c["do_sample"]:
        assert tok == ref.choose(v, do_sample=False)[0], row
        return
    want, keep, s = ref.choose(v, t=t, row=row, **c)
    assert want is not None and keep[tok], (row, tok, want)
    best = s[want]
    assert abs(s[tok] - best) <= TOL * max(1.0, abs(best)), (row, tok, want, s[tok], best)
    runner_up = np.sort(s[np.isfinite(s)])[-2] if np.isfinite(s).sum() > 1 else -np.inf
    if best - runner_up > 2 * TOL * max(1.0, abs(best)):
        assert tok == want, row


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_rows_equal_the_shared_form_row_by_row(ops, B, V):
    x = _logits(B, V, 7 * B + V)
    xd = x.cuda()
    cfg, t = _row_configs(B, V, B + V)
    got = ops.sample_tokens_rows(xd, t=t, **cfg).cpu().tolist()
    for r in range(B):
        shared = ops.sample_tokens(xd, t=t[r], **_row(cfg, r)).cpu().tolist()
        assert got[r] == shared[r], (r, _row(cfg, r), t[r])
        _check_ref(x[r].numpy(), got[r], _row(cfg, r), t[r], r)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_rows_with_processors_equal_the_shared_ex_form(ops, B, V):
    x = _logits(B, V, 11 * B + V)
    xd = x.cuda()
    cfg, t = _row_configs(B, V, 3 * B + V)
    rng = np.random.default_rng(V + B)
    pen = [float(rng.choice([0.5, 1.0, 1.3, 2.0])) for _ in range(B)]
    min_new = [int(rng.integers(0, 40)) for _ in range(B)]
    # (V = 1: a suppressed EOS would empty the row)
    eos = [(int(torch.argmax(x[r].float())), V - 1) if V > 2 else () for r in range(B)]
    seen = [rng.integers(0, V, int(rng.integers(0, 2 * V + 1))) for _ in range(B)]   # per-row histories, sparse to full
    before = pref.bitmap(seen, V)
    hist = torch.from_numpy(before.copy()).cuda()
    got = ops.sample_tokens_rows(xd, t=t, eos_ids=eos, repetition_penalty=pen, min_new_tokens=min_new, history=hist, **cfg).cpu().tolist()
    for r in range(B):
        h = torch.from_numpy(before.copy()).cuda()
        shared = ops.sample_tokens(xd, t=t[r], eos_ids=eos[r], repetition_penalty=pen[r], min_new_tokens=min_new[r], history=h,
                                   **_row(cfg, r)).cpu().tolist()
        assert got[r] == shared[r], (r, _row(cfg, r), t[r], pen[r], min_new[r])
        v = pref.process(x[r].numpy(), pref.seen_mask(before[r], V), t=t[r], repetition_penalty=pen[r], min_new_tokens=min_new[r],
                         eos_ids=eos[r])
        _check_ref(v, got[r], _row(cfg, r), t[r], r)
    want = before.view(np.uint32) | pref.bitmap([[o] for o in got], V).view(np.uint32)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want)


def _buffers(B, V, cap, t):
    return {"t": torch.tensor(t, dtype=torch.int32, device="cuda"),
            "out": torch.full((B,), -5, dtype=torch.int64, device="cuda"),
            "ring": torch.full((B, cap), -1, dtype=torch.int32, device="cuda"),
            "finished": torch.zeros(B, dtype=torch.int32, device="cuda"),
            "status": torch.zeros((B + 31) // 32, dtype=torch.int32, device="cuda")}


@pytest.mark.parametrize("proc", [False, True])
@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("B,V", [(1, 1), (3, 2047), (33, 2049), (33, 5000)])
def test_uniform_rows_equal_the_shared_launch(ops, B, V, do_sample, proc):
    """identical parameters and equal t: every word the launch writes equals the shared launch's, t[r] == *t, workspace zero"""
    x = _logits(B, V, B + V + 1)
    if V > 1:
        x[B - 1, V // 2] = float("nan")                       # a failed row: status bit, pad
    xd = x.cuda()
    eos = (int(torch.argmax(x[0].float())), 3) if V > 2 else ()
    cfg = dict(do_sample=do_sample, temperature=0.8, top_k=min(V, 20), top_p=0.95, seed=9, eos_ids=eos, pad=2)
    t0, cap = 4, 8
    seen = pref.bitmap([np.arange(r, V, 3) for r in range(B)], V)
    ws_bytes = ops.sample_workspace_bytes(B, V)
    s, r = _buffers(B, V, cap, [t0]), _buffers(B, V, cap, [t0] * B)
    for buf in (s, r):
        buf["finished"][B // 2] = 1 if B > 1 else 0            # an already finished row
        buf["ws"] = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        buf["hist"] = torch.from_numpy(seen.copy()).cuda()
    pk = (ops.sample_proc_params(1.3, 2).cuda(), ops.sample_proc_params_rows(B, 1.3, 2).cuda()) if proc else (None, None)
    ops.sample_launch(xd, ops.sample_params(**cfg).cuda(), s["t"], s["out"], s["status"], s["ws"], ring=s["ring"],
                      finished=s["finished"], proc=pk[0], history=s["hist"] if proc else None)
    ops.sample_launch_rows(xd, ops.sample_params_rows(B, **cfg).cuda(), r["t"], r["out"], r["status"], r["ws"], ring=r["ring"],
                           finished=r["finished"], proc=pk[1], history=r["hist"] if proc else None)
    torch.cuda.synchronize()
    for k in ("out", "ring", "finished", "status", "hist"):
        assert torch.equal(s[k], r[k]), k
    assert r["t"].cpu().tolist() == [int(s["t"].item())] * B == [t0 + 1] * B
    assert int(r["ws"].count_nonzero()) == 0 and int(s["ws"].count_nonzero()) == 0
    if V > 2:
        assert int(r["status"][(B - 1) // 32].item()) == 1 << ((B - 1) % 32)
    if V > 2 and not do_sample and not proc:
        assert int(r["finished"][0].item()) == 1               # row 0 emitted its EOS id


@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("V", [2047, 5000])
def test_per_row_bookkeeping(ops, V, do_sample):
    B, cap = 33, 12
    x = _logits(B, V, V + 5)
    x[torch.arange(B), torch.tensor([(37 * r + 11) % V for r in range(B)])] = 40.0   # one largest logit per row, no tie
    x[1] = x[0]                                                # rows 0 and 1 emit the same id (top_k = 1: the argmax)
    x[32, 100] = float("nan")
    tok0 = int(torch.argmax(x[0].float()))
    rng = np.random.default_rng(V)
    t = [int(v) for v in rng.integers(1, cap + 1, B)]
    eos = [()] * B
    eos[0] = (5, tok0)                                         # row 0 holds its token as EOS, row 1 does not
    pad = [100 + r for r in range(B)]
    max_new = [0] * B
    max_new[2], max_new[3], max_new[5] = t[2], t[3] + 1, -1    # at the budget / one before it / no budget
    buf = _buffers(B, V, cap, t)
    buf["finished"][4] = 1                                     # already finished
    st = ops.sample_tokens_rows(x.cuda(), do_sample=do_sample, top_k=1, seed=list(range(B)), t=buf["t"], eos_ids=eos, pad=pad,
                                out=buf["out"], ring=buf["ring"], finished=buf["finished"], status=buf["status"],
                                max_new_tokens=max_new)
    assert st is buf["out"]
    out, ring = buf["out"].cpu().tolist(), buf["ring"].cpu().numpy()
    argmax = torch.argmax(torch.nan_to_num(x.float(), nan=-1e9), -1).tolist()
    for r in range(B):
        want = pad[r] if r in (4, 32) else argmax[r]           # a finished and a NaN row emit their own pad
        assert out[r] == want, r
        row = np.full(cap, -1, dtype=np.int32)
        row[t[r] - 1] = want                                   # slot t[r] - 1 and no other
        assert np.array_equal(ring[r], row), r
    assert buf["t"].cpu().tolist() == [v + 1 for v in t]
    fin = buf["finished"].cpu().tolist()
    assert out[0] == out[1] == tok0 and fin[0] == 1 and fin[1] == 0
    assert fin[2] == 1 and out[2] == argmax[2]                 # the token at the budget is real, and the row latches
    assert fin[3] == 0 and fin[5] == 0
    assert fin[4] == 1 and fin[32] == 0                        # the NaN row does not latch
    assert sum(fin) == 3
    assert buf["status"].cpu().tolist() == [0, 1]              # row 32: bit 0 of word 1
    # the next launch: rows 0, 2 and 4 emit their pads, row 3 reaches its budget
    buf["status"].zero_()
    ops.sample_tokens_rows(x.cuda(), do_sample=do_sample, top_k=1, seed=list(range(B)), t=buf["t"], eos_ids=eos, pad=pad,
                           out=buf["out"], ring=buf["ring"], finished=buf["finished"], status=buf["status"], max_new_tokens=max_new)
    out, fin = buf["out"].cpu().tolist(), buf["finished"].cpu().tolist()
    assert [out[r] for r in (0, 2, 4, 32)] == [pad[0], pad[2], pad[4], pad[32]]
    assert out[3] == argmax[3] and fin[3] == 1 and fin[1] == 0 and fin[5] == 0
    assert buf["t"].cpu().tolist() == [v + 2 for v in t]       # finished rows keep advancing


@pytest.mark.parametrize("do_sample", [False, True])
def test_min_new_tokens_per_row(ops, do_sample):
    """the refilled slot: two rows with the same logits whose argmax is the EOS id, t = [1, 5], min_new_tokens = [3, 3] -- row 0
    is inside its window and must not emit EOS, row 1 is past it and must.  One shared t cannot do both."""
    V, eos = 5000, 4321
    x = _logits(1, V, 9).repeat(2, 1)
    x[:, eos] = 30.0
    x[:, 1234] = 20.0                                          # the one runner-up
    fin = torch.zeros(2, dtype=torch.int32, device="cuda")
    t = torch.tensor([1, 5], dtype=torch.int32, device="cuda")
    out = ops.sample_tokens_rows(x.cuda(), do_sample=do_sample, top_k=1, seed=1, t=t, eos_ids=[eos], pad=0, min_new_tokens=[3, 3],
                                 finished=fin).cpu().tolist()
    y = x[0].float().clone()
    y[eos] = -float("inf")
    assert out == [int(torch.argmax(y)), eos]
    assert fin.cpu().tolist() == [0, 1] and t.cpu().tolist() == [2, 6]
    # per-row windows at one token index
    t = torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    out = ops.sample_tokens_rows(x.cuda(), do_sample=do_sample, top_k=1, seed=1, t=t, eos_ids=[eos], pad=0, min_new_tokens=[3, 2]).cpu().tolist()
    assert out == [int(torch.argmax(y)), eos]


@pytest.mark.parametrize("B,V", [(3, 2049), (33, 5000)])
def test_graph_replay_with_parameters_rewritten_in_place(ops, B, V):
    """one captured rows launch replayed 6 times over changing logits; params, proc and max_new are rewritten in place between
    replays (rows switch between greedy and sampled); the result equals the eager loop"""
    n, cap = 6, 16
    xs = [_logits(B, V, 100 + i, scale=1.0) for i in range(n)]
    eos = [(int(torch.argmax(xs[2][r].float())),) if r % 2 else () for r in range(B)]
    rng = np.random.default_rng(B)
    steps = []
    for i in range(n):
        cfg, _ = _row_configs(B, V, 50 * B + i)
        steps.append((cfg, [float(rng.choice([1.0, 1.5])) for _ in range(B)], [int(rng.integers(0, 5)) for _ in range(B)]))
    max_new = [int(rng.integers(3, 12)) for _ in range(B)]
    t0 = [int(rng.integers(1, 5)) for _ in range(B)]
    max_new[0] = t0[0] + 2                                     # row 0 reaches its budget at the third launch
    seen = pref.bitmap([rng.integers(0, V, 30) for _ in range(B)], V)

    e = _buffers(B, V, cap, t0)
    e["hist"] = torch.from_numpy(seen.copy()).cuda()
    eager = []
    for i, (cfg, pen, mn) in enumerate(steps):
        eager.append(ops.sample_tokens_rows(xs[i].cuda(), t=e["t"], eos_ids=eos, pad=1, repetition_penalty=pen, min_new_tokens=mn,
                                            history=e["hist"], ring=e["ring"], finished=e["finished"], status=e["status"],
                                            max_new_tokens=max_new, **cfg).cpu())

    g = _buffers(B, V, cap, t0)
    g["hist"] = torch.from_numpy(seen.copy()).cuda()
    x = torch.zeros((B, V), dtype=torch.float16, device="cuda")
    params = torch.zeros((B, 64), dtype=torch.uint8, device="cuda")
    proc = torch.zeros((B, 16), dtype=torch.uint8, device="cuda")
    mx = torch.tensor(max_new, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.sample_workspace_bytes(B, V), dtype=torch.uint8, device="cuda")
    params.copy_(ops.sample_params_rows(B, eos_ids=eos, pad=1, **steps[0][0]))
    proc.copy_(ops.sample_proc_params_rows(B, steps[0][1], steps[0][2]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    replayed = []
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ops.sample_launch_rows(x, params, g["t"], g["out"], g["status"], ws, ring=g["ring"], finished=g["finished"], proc=proc,
                                   history=g["hist"], max_new=mx)
        for i, (cfg, pen, mn) in enumerate(steps):
            x.copy_(xs[i])
            params.copy_(ops.sample_params_rows(B, eos_ids=eos, pad=1, **cfg))
            proc.copy_(ops.sample_proc_params_rows(B, pen, mn))
            graph.replay()
            replayed.append(g["out"].cpu())
        s.synchronize()
    for i in range(n):
        assert torch.equal(replayed[i], eager[i]), i
    for k in ("t", "ring", "finished", "status", "hist"):
        assert torch.equal(g[k], e[k]), k
    assert g["t"].cpu().tolist() == [v + n for v in t0] and int(ws.count_nonzero()) == 0
    assert int(e["finished"].sum()) > 0                        # some row reached its budget or its EOS id
