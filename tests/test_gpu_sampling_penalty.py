"""The sampler's logit processors (csrc/sample.hip, awq_sample_tokens_ex) against the restatement sampling_ref.choose(
penalty_ref.process(...)) (MI355X).  Greedy is exact; a sampled token is checked as in tests/test_gpu_sampling.py.  Also: the
in-launch history update, EOS suppression while t <= min_new_tokens, p = 1 / min_new_tokens = 0 bitwise equal to
awq_sample_tokens, a captured graph replayed against the eager loop, the seed kernel, and saturated logits."""
import ctypes

import numpy as np
import pytest
import torch

import penalty_ref as pref
import sampling_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
CONFIGS = [None, {"temperature": 0.7, "top_k": 50, "top_p": 0.9}, {"temperature": 1.3, "top_k": 0, "top_p": 1.0}]


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import _lib, ops as o

    _lib.lib()
    return o


def _logits(B, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, V), generator=g) * scale).half()


def _seen_rows(B, V, seed):
    """row r: density r % 4 -- empty, a few ids, half, all"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(B):
        d = r % 4
        rows.append([] if d == 0 else rng.integers(0, V, 5) if d == 1 else rng.permutation(V)[:V // 2] if d == 2 else np.arange(V))
    return rows


def _check_sampled(v, tok, cfg, t, row, seed):
    want, keep, s = ref.choose(v, do_sample=True, seed=seed, t=t, row=row, **cfg)
    assert want is not None and keep[tok], (tok, want)
    best = s[want]
    assert abs(s[tok] - best) <= TOL * max(1.0, abs(best)), (tok, want, s[tok], best)
    runner_up = np.sort(s[np.isfinite(s)])[-2] if np.isfinite(s).sum() > 1 else -np.inf
    if best - runner_up > 2 * TOL * max(1.0, abs(best)):
        assert tok == want


def _sample(ops, x, hist, cfg, *, p, min_new=0, t=1, eos=(), seed=7, **kw):
    do_sample = cfg is not None
    return ops.sample_tokens(x.cuda(), do_sample=do_sample, seed=seed, t=t, eos_ids=eos, repetition_penalty=p,
                             min_new_tokens=min_new, history=hist, **(cfg or {}), **kw)


@pytest.mark.parametrize("V", [1, 7, 2049, 32000, 152064])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_tokens_equal_restatement(ops, B, V):
    x = _logits(B, V, B * 31 + V)
    rows = _seen_rows(B, V, V + B)
    for ci, cfg in enumerate(CONFIGS):
        if B == 64 and V > 32000 and ci == 2:
            continue  # (the fp64 restatement of 64 rows x 152k draws is the slow part; two configurations cover it)
        p, min_new, t = (1.3, 2, 2) if ci != 1 else (0.8, 0, 3)
        eos = [int(torch.argmax(x[0].float())), V - 1] if V > 2 else []   # (V = 1: a suppressed EOS would empty the row)
        before = pref.bitmap(rows, V)
        hist = torch.from_numpy(before.copy()).cuda()
        out = _sample(ops, x, hist, cfg, p=p, min_new=min_new, t=t, eos=eos, seed=ci + 3).cpu().numpy()
        for r in range(B):
            v = pref.process(x[r].numpy(), pref.seen_mask(before[r], V), t=t, repetition_penalty=p, min_new_tokens=min_new, eos_ids=eos)
            if cfg is None:
                assert int(out[r]) == ref.choose(v, do_sample=False)[0], (r, ci)
            else:
                _check_sampled(v, int(out[r]), cfg, t, r, ci + 3)
        after = hist.cpu().numpy().view(np.uint32)
        want = before.view(np.uint32) | pref.bitmap([[int(o)] for o in out], V).view(np.uint32)
        assert np.array_equal(after, want), ci


def test_history_update_includes_pads(ops):
    """before | bit(out) on every row: a finished row's pad and a bad row's pad too; a pad outside [0, V) sets nothing."""
    B, V = 5, 3000
    x = _logits(B, V, 3)
    x[2, 17] = float("nan")
    rows = _seen_rows(B, V, 1)
    for pad, do_sample in ((11, False), (12, True), (-1, False), (V, True)):
        before = pref.bitmap(rows, V)
        hist = torch.from_numpy(before.copy()).cuda()
        fin = torch.tensor([0, 1, 0, 0, 1], dtype=torch.int32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        cfg = {"top_k": 10} if do_sample else None
        out = _sample(ops, x, hist, cfg, p=1.1, pad=pad, finished=fin, status=status).cpu().numpy()
        assert out[1] == out[2] == out[4] == pad and int(status.item()) == 0b100
        want = before.view(np.uint32) | pref.bitmap([[int(o)] for o in out], V).view(np.uint32)
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), want), pad


@pytest.mark.parametrize("do_sample", [False, True])
def test_eos_suppressed_until_min_new_tokens(ops, do_sample):
    """EOS is the argmax by far; with min_new_tokens = 3 it is not emitted at t = 1 .. 3 and finished does not latch; at t = 4 it
    is emitted and latches."""
    B, V, eos = 3, 5000, 4321
    x = _logits(B, V, 9)
    x[:, eos] = 30.0
    xd = x.cuda()
    hist = torch.zeros((B, pref.words(V)), dtype=torch.int32, device="cuda")
    t = torch.ones(1, dtype=torch.int32, device="cuda")
    fin = torch.zeros(B, dtype=torch.int32, device="cuda")
    cfg = {"top_k": 1} if do_sample else {}
    for step in range(1, 5):
        out = ops.sample_tokens(xd, do_sample=do_sample, seed=1, t=t, eos_ids=[eos], pad=0, min_new_tokens=3, history=hist,
                                finished=fin, **cfg).cpu()
        if step <= 3:
            assert (out != eos).all() and int(fin.sum()) == 0, step
            if not do_sample:
                y = x.float().clone()
                y[:, eos] = -float("inf")
                assert out.tolist() == torch.argmax(y, -1).tolist()
        else:
            assert (out == eos).all() and fin.cpu().tolist() == [1] * B
    assert int(t.item()) == 5


@pytest.mark.parametrize("V", [1000, 152064])
def test_neutral_processors_equal_awq_sample_tokens(ops, V):
    """p = 1 and min_new_tokens = 0 through awq_sample_tokens_ex: the tokens of awq_sample_tokens bit for bit, whatever the
    history holds"""
    B = 8
    x = _logits(B, V, V).cuda()
    rows = _seen_rows(B, V, 2)
    for cfg in CONFIGS:
        base = ops.sample_tokens(x, do_sample=cfg is not None, seed=5, t=3, eos_ids=[1, 2], **(cfg or {})).cpu()
        hist = torch.from_numpy(pref.bitmap(rows, V)).cuda()
        got = ops.sample_tokens(x, do_sample=cfg is not None, seed=5, t=3, eos_ids=[1, 2], history=hist, **(cfg or {})).cpu()
        assert torch.equal(base, got)


@pytest.mark.parametrize("greedy", [True, False])
def test_graph_replay_equals_eager_loop(ops, greedy):
    """One captured processed launch replayed 16 times (t and the history advanced in the graph) against 16 eager calls."""
    B, V, n = 4, 2049, 16
    x = _logits(B, V, 77, scale=1.0).cuda()
    cfg = {"do_sample": False} if greedy else {"do_sample": True, "temperature": 0.9, "top_k": 40, "top_p": 0.95, "seed": 3}
    eos = [int(torch.argmax(x[1].float()))]
    prompt = _seen_rows(B, V, 4)

    eager_hist = torch.from_numpy(pref.bitmap(prompt, V)).cuda()
    eager = []
    for t in range(1, n + 1):
        eager.append(ops.sample_tokens(x, t=t, eos_ids=eos, repetition_penalty=1.5, min_new_tokens=3, history=eager_hist, **cfg).cpu())
    eager = torch.stack(eager, 1)

    params = ops.sample_params(eos_ids=eos, **cfg).cuda()
    proc = ops.sample_proc_params(1.5, 3).cuda()
    hist = torch.from_numpy(pref.bitmap(prompt, V)).cuda()
    t = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, dtype=torch.int64, device="cuda")
    ring = torch.full((B, n), -1, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.sample_workspace_bytes(B, V), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.sample_launch(x, params, t, out, status, ws, ring=ring, greedy=greedy, proc=proc, history=hist)
        for _ in range(n):
            g.replay()
        s.synchronize()
    assert int(t.item()) == n + 1 and int(status.item()) == 0 and int(ws.count_nonzero()) == 0
    assert torch.equal(ring.cpu().long(), eager)
    assert torch.equal(hist.cpu(), eager_hist.cpu())
    assert (eager[:, :3] != eos[0]).all()


def test_seed_kernel_equals_numpy_bitmap(ops):
    from autoawq_amd import _lib

    rng = np.random.default_rng(0)
    B, S, V = 5, 700, 40000
    ids = rng.integers(-50, V + 50, (B, S + 9))           # ids outside [0, V) are ignored by the kernel
    d = torch.from_numpy(ids).cuda()[:, 3:3 + S]           # row stride S + 9
    base = _seen_rows(B, V, 6)
    hist = torch.from_numpy(pref.bitmap(base, V, width=pref.words(V) + 3)).cuda()
    L = _lib.lib()
    rc = L.awq_sample_history_seed(hist.data_ptr(), hist.stride(0), d.data_ptr(), d.stride(0), B, S, V, None)
    assert rc == 0
    torch.cuda.synchronize()
    want = pref.bitmap([list(base[r]) + list(ids[r, 3:3 + S]) for r in range(B)], V, width=pref.words(V) + 3)
    assert np.array_equal(hist.cpu().numpy(), want)
    # the Python wrapper: a fresh history, then one extended in place
    ok = torch.from_numpy(rng.integers(0, V, (B, 33))).cuda()
    h = ops.sample_history(ok, V)
    assert np.array_equal(h.cpu().numpy(), pref.bitmap(ok.cpu().numpy(), V))
    more = torch.from_numpy(rng.integers(0, V, (B, 5))).cuda()
    ops.sample_history(more, V, out=h)
    assert np.array_equal(h.cpu().numpy(), pref.bitmap(np.concatenate([ok.cpu().numpy(), more.cpu().numpy()], 1), V))
    assert L.awq_sample_history_seed(hist.data_ptr(), pref.words(V) - 1, d.data_ptr(), d.stride(0), B, S, V, None) == -1


@pytest.mark.parametrize("p", [0.5, 2.0])
def test_saturated_logits_never_set_status(ops, p):
    B, V = 4, 4096
    x = torch.full((B, V), -65504.0).half()
    x[:, ::3] = 65504.0
    x[1, 7] = -float("inf")
    x[2] = -65504.0
    hist = torch.from_numpy(pref.bitmap([np.arange(V)] * B, V)).cuda()
    for cfg in CONFIGS:
        h = hist.clone()
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = _sample(ops, x, h, cfg, p=p, status=status).cpu().numpy()
        assert int(status.item()) == 0
        for r in range(B):
            v = pref.process(x[r].numpy(), np.ones(V, dtype=bool), repetition_penalty=p)
            assert np.isfinite(v[v > -np.inf]).all()
            if cfg is None:
                assert int(out[r]) == ref.choose(v, do_sample=False)[0]
            else:
                assert ref.choose(v, do_sample=True, seed=7, t=1, row=r, **cfg)[1][int(out[r])]


def test_launch_argument_checks(ops):
    from autoawq_amd import _lib

    x = _logits(2, 100, 1).cuda()
    params = ops.sample_params(do_sample=False).cuda()
    t = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.sample_workspace_bytes(2, 100), dtype=torch.uint8, device="cuda")
    proc = ops.sample_proc_params(1.2).cuda()
    with pytest.raises(_lib.AwqHipError):
        ops.sample_launch(x, params, t, out, status, ws, proc=proc)
    with pytest.raises(_lib.AwqHipError):
        ops.sample_launch(x, params, t, out, status, ws, proc=proc, history=torch.zeros((2, 3), dtype=torch.int32, device="cuda"))
    a = _lib.AwqSampleArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.logits, a.B, a.V, a.row_stride = x.data_ptr(), 2, 100, 100
    a.params, a.t, a.out, a.out_stride, a.status = params.data_ptr(), t.data_ptr(), out.data_ptr(), 1, status.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    q = _lib.AwqSampleProcArgs()
    q.struct_bytes = ctypes.sizeof(q)
    q.proc, q.history, q.history_stride = proc.data_ptr(), None, 4
    L = _lib.lib()
    assert L.awq_sample_tokens_ex(ctypes.byref(a), ctypes.byref(q)) == -6      # NULL history
    h = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    q.history, q.history_stride = h.data_ptr(), 3
    assert L.awq_sample_tokens_ex(ctypes.byref(a), ctypes.byref(q)) == -1      # stride < ceil(V / 32)
    q.history_stride, q.flags = 4, 1
    assert L.awq_sample_tokens_ex(ctypes.byref(a), ctypes.byref(q)) == -3      # reserved flags
    assert int(t.item()) == 1                                                  # nothing was launched
