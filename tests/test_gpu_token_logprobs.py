"""awq_token_logprobs (csrc/logprob.hip) on the MI355X against the fp64 reference, every element within the bound derived in
tests/logprob_bound.py (no extra factor): the vector and block boundaries of the kernel, both load paths, the contract's special
rows, needles at every thread / wave / step boundary, strided layouts, the slot form and a captured launch."""
import numpy as np
import pytest
import torch

import logprob_bound as lb

pytestmark = pytest.mark.gpu

# 8192 = the kernel's per-step width (1024 threads x 8 halves): 8191 / 8193 are that width -+ 1
VOCABS = (1, 7, 8, 9, 2047, 2048, 2049, 8191, 8193, 32000, 32003, 128256)
ROWS = (1, 3, 65)


def _gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _offset_by_one(x):
    """the same rows in a buffer whose base is one element past an allocation: no 16-byte loads possible"""
    R, V = x.shape
    flat = torch.empty(R * V + 1, dtype=torch.float16, device="cuda")
    flat[1:] = _gpu(x).view(-1)
    return flat[1:].view(R, V)


def _mixed_rows(R, V, seed):
    rng = np.random.default_rng(seed)
    x = np.stack([lb.make_row(lb.KINDS[(r + R) % len(lb.KINDS)], V, rng) for r in range(R)])
    ids = np.array([lb.targets(x[r])[(r // len(lb.KINDS)) % len(lb.targets(x[r]))] for r in range(R)], np.int64)
    return x, ids


@pytest.mark.parametrize("V", VOCABS)
def test_row_kinds_within_the_bound(V):
    from autoawq_amd import ops

    for R in ROWS:
        x, ids = _mixed_rows(R, V, 1000 * V + R)
        want, bound = lb.logprob_bound(x, ids)
        for path, lg in (("vector", _gpu(x)), ("element", _offset_by_one(x))):
            got = ops.token_logprobs(lg, _gpu(ids))
            assert got.dtype == torch.float32 and got.shape == (R,)
            worst = lb.assert_logprobs_close(got.cpu().numpy(), want, bound, f"V {V} R {R} {path}")
            print(f"V {V} R {R} {path}: worst error / bound {worst:.3f}")
        for r in range(R):   # flat rows: -log V within the bound
            if lb.KINDS[(r + R) % len(lb.KINDS)] == "flat":
                assert abs(float(got[r]) + np.log(V)) <= bound[r] + 1e-12


@pytest.mark.parametrize("V", (1, 7, 2049, 8193, 32003))
def test_contract_rows(V):
    from autoawq_amd import ops

    rng = np.random.default_rng(V)
    inf = np.float16(np.inf)
    base = lb.make_row("normal", V, rng)
    hot = V // 2
    one_hot = np.full(V, -inf, np.float16)
    one_hot[hot] = np.float16(3.5)
    own_inf = base.copy()
    own_inf[hot] = -inf                      # (V = 1: the row is then all -inf -> NaN)
    nan_row, pinf_row = base.copy(), base.copy()
    nan_row[V - 1] = np.float16(np.nan)
    pinf_row[0] = inf
    nan_among_inf = np.full(V, -inf, np.float16)
    nan_among_inf[V - 1] = np.float16(np.nan)
    x = np.stack([one_hot, own_inf, nan_row, pinf_row, np.full(V, -inf, np.float16), base, base, base, nan_among_inf])
    ids = np.array([hot, hot, 0, V - 1, 0, -1, V, hot, 0], np.int64)
    want, bound = lb.logprob_bound(x, ids)
    assert want[0] == 0.0 and (want[1] == -np.inf or V == 1) and np.isnan(want[[2, 3, 4, 6, 8]]).all() and want[5] == 0.0
    for path, lg in (("vector", _gpu(x)), ("element", _offset_by_one(x))):
        got = ops.token_logprobs(lg, _gpu(ids)).cpu().numpy()
        lb.assert_logprobs_close(got, want, bound, f"V {V} {path}")
        assert got[0] == 0.0 and got[5] == 0.0           # exactly: the one-hot row and the ignored slot
        assert np.isfinite(got[7])


def test_needles_at_every_thread_wave_and_step_boundary():
    """The second-largest logit, max - 1, at index 0, 7, 8, V - 1 and each side of every boundary of both load paths (vector:
    threads change every 8 elements, waves every 512, steps every 8192; element: slots every 1024, waves every 64): the reference
    without it lies > 100 bounds away, and the kernel is within the bound of the reference with it."""
    from autoawq_amd import ops

    V = 2 * lb.STEP + 9
    at = sorted({0, 7, 8, V - 1, 63, 64, 511, 512, 1023, 1024, lb.STEP - 1, lb.STEP, 2 * lb.STEP - 1, 2 * lb.STEP, 2 * lb.STEP + 7,
                 2 * lb.STEP + 8, lb.STEP + 511, lb.STEP + 512})
    rng = np.random.default_rng(5)
    base = np.clip(rng.standard_normal(V), -3.0, 3.0).astype(np.float16)
    top_at, scored = V // 2 + 3, V // 3
    assert top_at not in at and scored not in at
    x = np.repeat(base[None], len(at), 0)
    x[:, top_at] = np.float16(12.0)
    for r, e in enumerate(at):
        x[r, e] = np.float16(11.0)
    ids = np.full(len(at), scored, np.int64)
    want, bound = lb.logprob_bound(x, ids)
    without, _ = lb.logprob_bound(x, ids, drop=np.array(at))
    margin = lb.needle_margin(want, without, bound)
    assert margin.min() > 100, margin.min()
    for path, lg in (("vector", _gpu(x)), ("element", _offset_by_one(x))):
        got = ops.token_logprobs(lg, _gpu(ids)).cpu().numpy()
        worst = lb.assert_logprobs_close(got, want, bound, path)
        print(f"needles, {path}: worst error / bound {worst:.3f}, least margin {margin.min():.0f} bounds")
    # ... and scoring the needle itself
    ids = np.array(at, np.int64)
    want, bound = lb.logprob_bound(x, ids)
    lb.assert_logprobs_close(ops.token_logprobs(_gpu(x), _gpu(ids)).cpu().numpy(), want, bound, "needle as the id")


@pytest.mark.parametrize("V", (2048, 2049))
def test_strided_rows_ids_and_leading_dimensions(V):
    from autoawq_amd import ops

    B, T = 5, 3
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((B, T, V)) * 2.0).astype(np.float16)
    ids = rng.integers(0, V, (B, T))
    big = _gpu(x)
    # the last position of [B, T, V]: a row stride of T V elements, nothing copied
    want, bound = lb.logprob_bound(x[:, -1], ids[:, -1])
    got = ops.token_logprobs(big[:, -1], _gpu(ids[:, -1]))
    lb.assert_logprobs_close(got.cpu().numpy(), want, bound, "last position")
    # ids with a stride, through the raw launch (which takes the last position of [B, T, V] itself)
    out = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ops.token_logprobs_launch(big, _gpu(ids)[:, -1], out)
    assert torch.equal(out, got)
    # all leading dimensions at once, and leading dimensions that do not collapse to one stride
    want, bound = lb.logprob_bound(x.reshape(B * T, V), ids.reshape(-1))
    got = ops.token_logprobs(big, _gpu(ids))
    assert got.shape == (B, T)
    lb.assert_logprobs_close(got.cpu().numpy(), want, bound, "[B, T, V]")
    want, bound = lb.logprob_bound(x[:, ::2].reshape(B * 2, V), ids[:, ::2].reshape(-1))
    got = ops.token_logprobs(big[:, ::2], _gpu(ids)[:, ::2])
    lb.assert_logprobs_close(got.cpu().numpy(), want, bound, "[B, ::2, V]")
    pre = torch.empty((B, 2), dtype=torch.float32, device="cuda")
    assert ops.token_logprobs(big[:, ::2], _gpu(ids)[:, ::2], out=pre) is pre and torch.equal(pre, got)
    # no rows: nothing launched
    assert ops.token_logprobs(big[:0], _gpu(ids)[:0]).shape == (0, T)


def test_slot_form_fills_a_ring_and_drops_writes_past_its_capacity():
    from autoawq_amd import ops

    R, V, cap = 3, 2049, 2
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((R, V)) * 2.0).astype(np.float16)
    lg = _gpu(x)
    buf = torch.full((R, 4), 777.0, dtype=torch.float32, device="cuda")   # canaries in columns 0 and 3 around out = columns 1 .. 2
    out = buf[:, 1:1 + cap]
    slot = torch.zeros(R, dtype=torch.int32, device="cuda")
    calls = [np.array([5, -1, V - 1]), np.array([0, 9, 10]), np.array([1, 2, 3])]
    for i, ids in enumerate(calls):
        ops.token_logprobs_launch(lg, _gpu(ids.astype(np.int64)), out, slot=slot)
        assert slot.tolist() == [i + 1] * R                               # the slots advance, dropped write or not
    got = buf.cpu().numpy()
    assert (got[:, 0] == 777.0).all() and (got[:, 3] == 777.0).all()      # the third launch wrote nothing
    for i in range(cap):
        want, bound = lb.logprob_bound(x, calls[i])
        lb.assert_logprobs_close(got[:, 1 + i], want, bound, f"slot {i}")
    assert got[1, 1] == 0.0                                               # the ignored slot still takes its column


def test_captured_launch_replays_on_changed_logits():
    from autoawq_amd import ops

    R, V = 2, 8193
    rng = np.random.default_rng(9)
    xs = [(rng.standard_normal((R, V)) * 2.0).astype(np.float16) for _ in range(2)]
    lg = _gpu(xs[0]).clone()
    ids = _gpu(np.array([[3], [V - 1]], np.int64))                        # [R, 1]: a decoder's token buffer
    out = torch.zeros((R, 4), dtype=torch.float32, device="cuda")
    slot = torch.zeros(R, dtype=torch.int32, device="cuda")
    ops.token_logprobs_launch(lg, ids, out, slot=slot)                    # warm-up outside the capture
    torch.cuda.synchronize()
    out.zero_()
    slot.zero_()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            ops.token_logprobs_launch(lg, ids, out, slot=slot)
    torch.cuda.synchronize()
    assert slot.tolist() == [0, 0]                                        # recorded, not run
    for x in xs:
        lg.copy_(_gpu(x))
        graph.replay()
    torch.cuda.synchronize()
    assert slot.tolist() == [2, 2]
    got = out.cpu().numpy()
    for i, x in enumerate(xs):
        want, bound = lb.logprob_bound(x, [3, V - 1])
        lb.assert_logprobs_close(got[:, i], want, bound, f"replay {i}")
    assert (got[:, 2:] == 0.0).all()


def test_row_offsets_past_2_to_the_31_elements():
    """R V > 2^31: the last row starts at element 2^31 of the tensor.  Every other row is an ignored slot and is not read."""
    from autoawq_amd import ops

    V, R = 1 << 20, 2049
    rng = np.random.default_rng(31)
    row = (rng.standard_normal(V) * 2.0).astype(np.float16)
    lg = torch.empty((R, V), dtype=torch.float16, device="cuda")
    lg[-1] = _gpu(row)
    ids = torch.full((R,), -1, dtype=torch.int64, device="cuda")
    ids[-1] = V - 1
    got = ops.token_logprobs(lg, ids).cpu().numpy()
    assert (got[:-1] == 0.0).all()
    want, bound = lb.logprob_bound(row, [V - 1])
    lb.assert_logprobs_close(got[-1:], want, bound, "row 2048 of 2^20 columns")
