"""The sampler's slots form (awq_sample_tokens_slots, csrc/sample.hip) and awq_spec_accept_ex (csrc/spec.hip) on MI355X.

Contract E1, exactly: slot (b, j) of a B x T launch -- its token and its status bit -- equals row b of a B-row launch of
awq_sample_tokens_rows on the slots' logits rows with t[b] = cnt[b] + 1 + j, the same params / proc and history row b with the
bits of tok[b, 1 .. j] ORed in.  V on both sides of the sampler's 2048-element chunk and of a history word, T in {2, 3, 8}, B in
{1, 3}, B * T = 1024; random logits, heavy ties, -inf runs, a NaN row, an all -inf row; drafts at the history word edges,
repeated, already seen, an EOS id while the min_new_tokens window closes inside the row's slots, and outside [0, V).

Against the fp64 restatement (tests/spec_sample_ref.py) a sampled token is held as tests/test_gpu_sampling_rows.py holds one
(_check_ref and its TOL: in the kept set, its score within TOL of the best, equal where the best leads by more than 2 TOL).  Those
tests cap no share of non-decisive rows -- the rule is checked on every row -- so the share is printed and held to the quarter
that the suite's other margin rule allows (tests/test_gpu_spec_generate.py).  Measured on MI355X: 0 of 48 slots (0.000)."""
import numpy as np
import pytest
import torch

import penalty_ref as pref
import spec_ref
import spec_sample_ref as sref
from test_gpu_sampling_rows import TOL, _check_ref

pytestmark = pytest.mark.gpu
KINDS = ["random", "ties", "neg_inf_runs", "nan_row", "all_neg_inf_row"]


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import _lib, ops as o

    _lib.lib()
    return o


def _logits(kind, R, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, V), generator=g) * 3.0
    if kind == "ties":
        x = torch.tensor([-2.0, -0.5, 0.0, 1.0, 2.5])[torch.randint(0, 5, (R, V), generator=g)]
    x = x.half()
    if kind == "neg_inf_runs":
        for r in range(R):
            a = (7 * r + 3) % V
            x[r, a:a + max(1, V // 3)] = -float("inf")
            x[r, :V // 5] = -float("inf")
    if kind == "nan_row":
        x[R - 1, V // 2] = float("nan")
    if kind == "all_neg_inf_row":
        x[R // 2] = -float("inf")
    return x


def _case(kind, B, T, V, seed, finished_row=None):
    """one launch's inputs on the CPU: logits [B * T, V], per-request parameters (greedy and sampled mixed), cnt, tok, history"""
    rng = np.random.default_rng(seed)
    x = _logits(kind, B * T, V, seed)
    cnt = rng.integers(1, 30, B).astype(np.int32)
    seen = [rng.integers(0, V, int(rng.integers(1, V + 1))) for _ in range(B)]
    hist_id = [int(s[0]) for s in seen]
    eos_draft = (V // 2) % V
    tok = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        # id 0, the history word edges 31 / 32, V - 1, a repeat, an id the history holds, an EOS id, ids outside [0, V)
        pool = [0, 31 % V, 32 % V, V - 1, 32 % V, hist_id[b], eos_draft, V + 3, -1]
        tok[b, 0] = hist_id[b]
        for i in range(T - 1):
            tok[b, 1 + i] = pool[(2 * b + KINDS.index(kind) + i) % len(pool)]
    seen = [np.append(s, tok[b, 0]) for b, s in enumerate(seen)]     # tok[b, 0] is in the history already
    if kind in ("random", "ties"):      # the drafts near the top of their rows: whether they count as seen decides the token
        for b in range(B):
            for j in range(T):
                for d in tok[b, 1:]:
                    if 0 <= d < V:
                        x[b * T + j, d] = 9.0 + 0.25 * (int(d) % 5)
    # the min_new_tokens window closes inside the row's slots: slots 0 .. (T - 1) // 2 are suppressed, the later ones are not
    min_new = [int(cnt[b]) + 1 + (T - 1) // 2 for b in range(B)]
    eos = [(int(torch.argmax(torch.nan_to_num(x[b * T].float(), nan=-1e9))), eos_draft) for b in range(B)]
    cfg = {"do_sample": [b % 3 != 1 for b in range(B)], "temperature": [[0.7, 1.0, 1.4][b % 3] for b in range(B)],
           "top_k": [[0, 5, max(1, V // 3)][(b + seed) % 3] for b in range(B)], "top_p": [[1.0, 0.9, 0.5][(b + T) % 3] for b in range(B)],
           "seed": [int(s) for s in rng.integers(0, 2 ** 62, B)], "eos_ids": eos, "pad": [V + 10 + b for b in range(B)]}
    proc = {"repetition_penalty": [[1.3, 2.0, 0.5][b % 3] for b in range(B)], "min_new_tokens": min_new}
    finished = np.zeros(B, dtype=np.int32)
    if finished_row is not None:
        finished[finished_row] = 1
    return {"x": x, "cnt": cnt, "tok": tok, "hist": pref.bitmap(seen, V), "cfg": cfg, "proc": proc, "finished": finished}


def _run_slots(ops, c, B, T, V, use_proc=True, greedy=False):
    """the slots launch on clones; asserts that it wrote nothing but pred / status and left the workspace zero"""
    d = {"x": c["x"].cuda(), "cnt": torch.from_numpy(c["cnt"]).cuda(), "tok": torch.from_numpy(c["tok"]).cuda(),
         "hist": torch.from_numpy(c["hist"].copy()).cuda(), "finished": torch.from_numpy(c["finished"]).cuda()}
    pred = torch.full((B * T,), -7, dtype=torch.int64, device="cuda")
    status = torch.zeros((B * T + 31) // 32, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.sample_workspace_bytes(B * T, V), dtype=torch.uint8, device="cuda")
    ops.sample_launch_slots(d["x"], ops.sample_params_rows(B, **c["cfg"]).cuda(), d["cnt"], d["tok"], pred, status, ws,
                            finished=d["finished"], greedy=greedy,
                            proc=ops.sample_proc_params_rows(B, **c["proc"]).cuda() if use_proc else None,
                            history=d["hist"] if use_proc else None)
    torch.cuda.synchronize()
    assert int(ws.count_nonzero()) == 0
    assert np.array_equal(d["cnt"].cpu().numpy(), c["cnt"]) and np.array_equal(d["tok"].cpu().numpy(), c["tok"])
    assert np.array_equal(d["hist"].cpu().numpy(), c["hist"]) and np.array_equal(d["finished"].cpu().numpy(), c["finished"])
    assert torch.equal(d["x"].cpu().view(torch.int16), c["x"].view(torch.int16))
    st = status.cpu().numpy().view(np.uint32)
    bits = np.array([(int(st[r // 32]) >> (r % 32)) & 1 for r in range(B * T)]).reshape(B, T)
    return pred.cpu().numpy().reshape(B, T), bits


def _run_rows(ops, c, B, T, V, use_proc=True, greedy=False):
    """E1's right-hand side: for every j one B-row launch of the rows form -> (tokens [B, T], status bits [B, T])"""
    xd = c["x"].cuda().view(B, T, V)
    params = ops.sample_params_rows(B, **c["cfg"]).cuda()
    proc = ops.sample_proc_params_rows(B, **c["proc"]).cuda() if use_proc else None
    ws = torch.zeros(ops.sample_workspace_bytes(B, V), dtype=torch.uint8, device="cuda")
    toks, bits = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for j in range(T):
        hist = c["hist"].view(np.uint32) | pref.bitmap([c["tok"][b, 1:j + 1] for b in range(B)], V, c["hist"].shape[1]).view(np.uint32)
        out = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        status = torch.zeros((B + 31) // 32, dtype=torch.int32, device="cuda")
        ops.sample_launch_rows(xd[:, j].contiguous(), params, torch.from_numpy((c["cnt"] + 1 + j).astype(np.int32)).cuda(), out, status, ws,
                               finished=torch.from_numpy(c["finished"].copy()).cuda(), greedy=greedy, proc=proc,
                               history=torch.from_numpy(hist.view(np.int32).copy()).cuda() if use_proc else None)
        st = status.cpu().numpy().view(np.uint32)
        toks[:, j] = out.cpu().numpy()
        bits[:, j] = [(int(st[b // 32]) >> (b % 32)) & 1 for b in range(B)]
    return toks, bits


def _e1(ops, c, B, T, V, **kw):
    got, got_bits = _run_slots(ops, c, B, T, V, **kw)
    want, want_bits = _run_rows(ops, c, B, T, V, **kw)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(got_bits, want_bits)
    return got, got_bits


@pytest.mark.parametrize("V", [33, 2048, 2049, 4100])
@pytest.mark.parametrize("T", [2, 3, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_e1_slots_equal_the_rows_form(ops, B, T, V):
    pads = 0
    for k, kind in enumerate(KINDS):
        c = _case(kind, B, T, V, 1000 * B + 100 * T + V + k)
        got, bits = _e1(ops, c, B, T, V)
        if kind == "nan_row":
            assert bits[B - 1, T - 1] == 1 and got[B - 1, T - 1] == c["cfg"]["pad"][B - 1]
        if kind == "all_neg_inf_row":
            r = (B * T) // 2
            assert bits[r // T, r % T] == 1 and got[r // T, r % T] == c["cfg"]["pad"][r // T]
        if kind in ("random", "ties"):
            assert bits.sum() == 0
        pads += int(bits.sum())
    assert pads >= 2
    c = _case("random", B, T, V, 77 * B + T + V)
    _e1(ops, c, B, T, V, use_proc=False)                       # proc = NULL: the kernels that read neither proc nor history
    _e1(ops, c, B, T, V, greedy=True)                          # AWQ_SAMPLE_FLAG_GREEDY: argmax whatever the parameters say
    _e1(ops, c, B, T, V, use_proc=False, greedy=True)
    c = _case("ties", B, T, V, 5 * B + T + V, finished_row=B - 1)
    got, bits = _e1(ops, c, B, T, V)                           # a finished request: pad in every slot, no status bit
    assert (got[B - 1] == c["cfg"]["pad"][B - 1]).all() and bits[B - 1].sum() == 0


def test_e1_at_1024_rows(ops):
    B, T, V = 128, 8, 64
    c = _case("random", B, T, V, 9, finished_row=17)
    got, bits = _e1(ops, c, B, T, V)
    assert (got[17] == c["cfg"]["pad"][17]).all() and bits.sum() == 0
    c = _case("nan_row", B, T, V, 10)
    got, bits = _e1(ops, c, B, T, V)
    assert bits[B - 1, T - 1] == 1 and bits.sum() == 1          # bit 1023: the last bit of the last status word


def test_the_drafts_in_front_of_a_slot_count_as_seen(ops):
    """greedy, penalty 2, logits 10 / 9 / 8.9 at ids 5 / 6 / 7 in every slot, drafts 5 and 6: slot 0 takes 5; slot 1 sees 5 halved
    and takes 6; slot 2 sees 5 and 6 halved and takes 7.  The history alone (id 1) would give 5 three times."""
    V, T = 64, 3
    x = torch.zeros((T, V), dtype=torch.float16)
    x[:, 5], x[:, 6], x[:, 7] = 10.0, 9.0, 8.9
    tok = torch.tensor([[1, 5, 6]], dtype=torch.int64).cuda()
    cnt = torch.tensor([4], dtype=torch.int32).cuda()
    hist = ops.sample_history(tok[:, :1], V)
    pred = ops.sample_tokens_slots(x.cuda().view(1, T, V), tok, cnt, do_sample=False, repetition_penalty=2.0, history=hist)
    assert pred.cpu().tolist() == [[5, 6, 7]]
    assert np.array_equal(hist.cpu().numpy(), pref.bitmap([[1]], V))
    pred = ops.sample_tokens_slots(x.cuda().view(1, T, V), tok, cnt, do_sample=True, top_k=1, seed=3, repetition_penalty=2.0, history=hist)
    assert pred.cpu().tolist() == [[5, 6, 7]]


def test_slots_against_the_fp64_reference(ops):
    B, T, V = 3, 4, 2049
    total = loose = 0
    for seed in range(4):
        c = _case("random", B, T, V, 300 + seed)
        got, bits = _run_slots(ops, c, B, T, V)
        assert bits.sum() == 0
        for b in range(B):
            cfg = {k: v[b] for k, v in c["cfg"].items() if k not in ("eos_ids", "pad")}
            proc = {k: v[b] for k, v in c["proc"].items()}
            for j in range(T):
                v = sref.slot_logits(c["x"][b * T + j].numpy(), c["hist"][b], c["tok"][b], j, c["cnt"][b], eos_ids=c["cfg"]["eos_ids"][b], **proc)
                t = int(c["cnt"][b]) + 1 + j
                _check_ref(v, int(got[b, j]), cfg, t, b)
                want, _, s = sref.slot_choose(c["x"][b * T + j].numpy(), c["hist"][b], c["tok"][b], j, c["cnt"][b], b,
                                              eos_ids=c["cfg"]["eos_ids"][b], **cfg, **proc)
                total += 1
                if s is not None:
                    top = np.sort(s[np.isfinite(s)])[-2:]
                    loose += bool(top[1] - top[0] <= 2 * TOL * max(1.0, abs(top[1])))
    print(f"slots vs fp64: {loose} of {total} slots are not decisive ({loose / total:.3f})")
    assert loose / total <= 0.25


# ---- awq_spec_accept_ex -----------------------------------------------------------------------------------------------------------

def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _accept_case(T, V, seed):
    rng = np.random.default_rng(seed)
    B, ring_cap, hist_cap, max_new = 9, 40, 90, 30
    eos = (3, 11)
    edge = [0, 31, 32, 63, 64, V - 1, V - 2, 33]
    tok = rng.integers(12, V, size=(B, T)).astype(np.int64)
    pred = rng.integers(12, V, size=(B, T)).astype(np.int64)
    pred[0, :T - 1] = tok[0, 1:]                               # row 0: every draft accepted
    pred[1, :T - 1] = tok[1, 1:]                               # row 1: an EOS inside the accepted run
    pred[1, (T - 1) // 2] = 11
    if (T - 1) // 2 < T - 1:
        tok[1, (T - 1) // 2 + 1] = 11
    pred[2, :T - 1] = tok[2, 1:]                               # row 2: the budget ends the run after one token
    pred[3, :T - 1] = tok[3, 1:]                               # row 3: a status bit in one slot
    pred[4, :T - 1] = tok[4, 1:]                               # row 4: finished
    pred[5] = [edge[i % len(edge)] for i in range(T)]          # row 5: ids at the history word edges, all accepted
    tok[5, 1:] = pred[5, :T - 1]
    pred[6, 0] = V + 5                                         # row 6: an id outside [0, V) (a pad), then a rejected draft
    tok[6, 1] = 13 if pred[6, 0] != 13 else 14
    pred[7, 0] = (tok[7, 1] + 1 - 12) % (V - 12) + 12          # row 7: the first draft rejected
    state = {"hist": rng.integers(0, V, size=(B, hist_cap)).astype(np.int32),
             "n_hist": rng.integers(1, 50, size=B).astype(np.int32),
             "cnt": rng.integers(1, max_new - T - 1, size=B).astype(np.int32),
             "ring": rng.integers(0, V, size=(B, ring_cap)).astype(np.int32),
             "finished": np.zeros(B, dtype=np.int32),
             "pos_rows": rng.integers(0, 100, size=B).astype(np.int32),
             "len_rows": rng.integers(0, 100, size=B).astype(np.int32)}
    state["cnt"][2] = max_new - 1
    state["finished"][4] = 1
    bad = np.zeros(B, dtype=bool)
    bad[3] = True
    status = np.zeros((B * T + 31) // 32, dtype=np.int64)
    r = 3 * T + T - 1
    status[r // 32] |= 1 << (r % 32)
    history = pref.bitmap([rng.integers(0, V, 10) for _ in range(B)], V, pref.words(V) + 1)   # a stride wider than ceil(V / 32)
    return tok, pred, state, bad, status.astype(np.uint32).view(np.int32), history, {"max_new_tokens": max_new, "eos": eos}


@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("V", [65, 2049])
def test_accept_ex_equals_the_reference(ops, T, V):
    tok, pred, state, bad, status, history, par = _accept_case(T, V, 10 * T + V)
    params = ops.spec_params(eos_ids=par["eos"], max_new_tokens=par["max_new_tokens"], ngram_max=2).cuda()
    runs = {}
    for name in ("ex", "plain"):
        dev = {k: _dev(v, torch.int32) for k, v in state.items()}
        dev["history"] = _dev(history, torch.int32)
        more = {"history": dev["history"], "vocab": V} if name == "ex" else {}
        tok_d = _dev(tok, torch.int64)
        ops.spec_accept(params, tok_d, _dev(pred.reshape(-1), torch.int64), dev["hist"], dev["n_hist"], dev["cnt"], dev["ring"],
                        dev["finished"], dev["pos_rows"], dev["len_rows"], status=_dev(status, torch.int32), **more)
        assert np.array_equal(tok_d.cpu().numpy(), tok)
        runs[name] = {k: v.cpu().numpy() for k, v in dev.items()}
    want_hist = history.copy()
    emitted = sref.accept_state(state, tok, pred, par, status_bad=bad, history=want_hist, V=V)
    for name, want in state.items():
        assert np.array_equal(runs["ex"][name], want), name
        assert np.array_equal(runs["plain"][name], want), name    # a NULL second argument is awq_spec_accept
    assert np.array_equal(runs["ex"]["history"], want_hist)
    assert np.array_equal(runs["plain"]["history"], history)
    assert len(emitted[0]) == T and emitted[1][-1] == 11 and len(emitted[1]) == (T - 1) // 2 + 1 and len(emitted[2]) == 1
    assert emitted[3] == [] and emitted[4] == [] and emitted[5] == [int(p) for p in pred[5]] and emitted[6] == [V + 5]
    assert len(emitted[7]) == 1
    assert np.array_equal(want_hist[[3, 4, 6]], history[[3, 4, 6]])   # status bit, finished, out of range: no bit moves


# ---- the three launches together ------------------------------------------------------------------------------------------------

def _spec_words(ops, B, T, V, prompt, max_new):
    """the device words of a speculative run after token 1 (the prompt's last id stands for it): as decode.py sets them up"""
    w = {"tok": torch.zeros((B, T), dtype=torch.int64, device="cuda"), "pred": torch.zeros(B * T, dtype=torch.int64, device="cuda"),
         "status": torch.zeros((B * T + 31) // 32, dtype=torch.int32, device="cuda"),
         "ws": torch.zeros(ops.sample_workspace_bytes(B * T, V), dtype=torch.uint8, device="cuda"),
         "hist": torch.zeros((B, 256), dtype=torch.int32, device="cuda"), "n_hist": torch.zeros(B, dtype=torch.int32, device="cuda"),
         "cnt": torch.ones(B, dtype=torch.int32, device="cuda"), "ring": torch.zeros((B, 64), dtype=torch.int32, device="cuda"),
         "finished": torch.zeros(B, dtype=torch.int32, device="cuda"), "pos": torch.zeros(B, dtype=torch.int32, device="cuda"),
         "len": torch.ones(B, dtype=torch.int32, device="cuda"),
         "params": ops.spec_params(max_new_tokens=max_new, ngram_max=2).cuda()}
    p = torch.tensor(prompt, dtype=torch.int64).cuda()
    w["hist"][:, :p.shape[1]] = p.to(torch.int32)
    w["n_hist"].fill_(p.shape[1])
    w["history"] = ops.sample_history(p, V)
    ops.ngram_draft(w["params"], w["tok"], w["hist"], w["n_hist"])
    return w


def _round(ops, w, x, sparams, proc, V):
    ops.sample_launch_slots(x, sparams, w["cnt"], w["tok"], w["pred"], w["status"], w["ws"], finished=w["finished"], proc=proc,
                            history=w["history"])
    ops.spec_accept(w["params"], w["tok"], w["pred"], w["hist"], w["n_hist"], w["cnt"], w["ring"], w["finished"], w["pos"], w["len"],
                    status=w["status"], history=w["history"], vocab=V)
    ops.ngram_draft(w["params"], w["tok"], w["hist"], w["n_hist"])


@pytest.mark.parametrize("T", [2, 8])
def test_peaked_logits_emit_every_slot(ops, T):
    """one logit 30 above the rest per slot, the drafts equal to the peaks, sampled at temperature 1: p(draft) = 1 up to e^-30 V,
    every request emits T tokens and its history gains exactly those bits"""
    B, V = 3, 2049
    peaks = np.array([[(97 * b + 31 * j + 32) % V for j in range(T)] for b in range(B)])
    x = _logits("random", B * T, V, T).view(B, T, V) * 0.1
    for b in range(B):
        for j in range(T):
            x[b, j, peaks[b, j]] = 30.0
    w = _spec_words(ops, B, T, V, [[1, 2], [3, 4], [5, 6]], 40)
    w["tok"][:, 1:] = torch.from_numpy(peaks[:, :T - 1]).cuda()
    before = w["history"].cpu().numpy().copy()
    _round(ops, w, x.cuda(), ops.sample_params_rows(B, do_sample=True, temperature=1.0, seed=[4, 5, 6]).cuda(),
           ops.sample_proc_params_rows(B, 1.2, 0).cuda(), V)
    assert w["cnt"].cpu().tolist() == [1 + T] * B
    assert np.array_equal(w["ring"][:, 1:1 + T].cpu().numpy(), peaks)
    want = before.view(np.uint32) | pref.bitmap(list(peaks), V).view(np.uint32)
    assert np.array_equal(w["history"].cpu().numpy().view(np.uint32), want)
    assert int(w["status"].count_nonzero()) == 0 and int(w["ws"].count_nonzero()) == 0


def test_one_capture_replayed_equals_eager_rounds(ops):
    """slots -> accept_ex -> draft captured once and replayed 3 times on fixed logits: cnt, history and the drafts advance on the
    device between replays, so the three rounds differ, and they equal 3 eager rounds"""
    B, T, V = 3, 4, 2049
    x = (_logits("random", B * T, V, 21) * 0.5).cuda()
    prompt = [[7, 8, 7, 8, 7], [1, 2, 3, 1, 2], [9, 9, 9, 9, 9]]
    sparams = ops.sample_params_rows(B, do_sample=[True, True, False], temperature=[0.8, 1.2, 1.0], top_k=[0, 50, 0], seed=[1, 2, 3]).cuda()
    proc = ops.sample_proc_params_rows(B, [1.3, 1.0, 1.5], [0, 3, 0]).cuda()
    e = _spec_words(ops, B, T, V, prompt, 40)
    for _ in range(3):
        _round(ops, e, x, sparams, proc, V)
    g = _spec_words(ops, B, T, V, prompt, 40)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            _round(ops, g, x, sparams, proc, V)
        for _ in range(3):
            graph.replay()
        s.synchronize()
    for k in ("tok", "pred", "status", "hist", "n_hist", "cnt", "ring", "finished", "pos", "len", "history"):
        assert torch.equal(g[k], e[k]), k
    cnt = e["cnt"].cpu().tolist()
    assert all(4 <= c <= 1 + 3 * T for c in cnt) and int(g["ws"].count_nonzero()) == 0
    assert int(e["history"].count_nonzero()) > 0
