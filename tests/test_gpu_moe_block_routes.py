"""The fused MoE block (modules/fused/moe.py::apply_moe_weights, ep.apply_moe_weights_local) on CRAFTED routing -- every token on
the same two experts, exact ties, a routing weight of 1e-26, experts nobody chose, expert counts that fill the padded capacity or
leave no padding -- at the pair counts on both sides of each hand-over of the dispatch: ROWS_MAX_PAIRS (12 | 14), DECODE_MAX_PAIRS
(64 | 66: 8-row to 16-row blocks) and PREFILL_MIN_PAIRS (382 | 384), on two copies with and without decode twins and on the
single copy.  The reference is oracle.moe_forward, the tolerance the block's own (tests/test_gpu_moe_rows.py): a pair computed by
the wrong expert, written to the wrong slot or row, or weighted with its neighbour's weight is an error of the order of the
output's rms, hundreds of times that tolerance.
Shapes of tests/test_gpu_moe_rows.py: E = 8, H = 512, I = 768, g = 128, top-2; and one E = 4, top-4 stack (every expert, every token)."""
import numpy as np
import pytest
import torch

import moe_route_ref as mr
from test_gpu_moe_rows import Stack, gemm_stacks

pytestmark = pytest.mark.gpu

H, I, G = 512, 768, 128
FAMILIES = ("crowded", "all_equal", "spread60", "empties", "multiple", "one_mod_block")
T_TOP2 = (6, 7, 32, 33, 191, 192)   # 12 | 14, 64 | 66, 382 | 384 pairs
T_TOP4 = (3, 4, 16, 17)             # 12 | 16, 64 | 68 pairs
CROWD = (5, 2)                      # crowded's two experts: of ranks 2 and 1 when four ranks share eight experts


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()  # fails loudly if the extension is missing
    return _ops


def block_logits(E, topk, fam, T):
    """fp32 logits [T, E], or None where T cannot carry the family (the two built from expert counts, for the block the dispatch
    aligns with at this T)"""
    block = 8 if T * topk <= 64 else 16
    if fam == "spread60":
        lg = mr.build("spread", T, E, topk, T, second=-60.0)
    elif fam == "crowded":
        lg = mr.build(fam, T, E, topk, T, top=CROWD if E == 8 else None)
    else:
        lg = mr.build(fam, T, E, topk, T, block=block)
    assert lg is None or mr.decidable(lg), (fam, T)
    return lg


TOP2_CASES = [(T, fam) for T in T_TOP2 for fam in FAMILIES if block_logits(8, 2, fam, T) is not None]
TOP4_CASES = [(T, fam) for T in T_TOP4 for fam in FAMILIES if block_logits(4, 4, fam, T) is not None]
assert all((T, fam) in TOP2_CASES for T in T_TOP2 for fam in FAMILIES[:4]) and {(32, "multiple"), (32, "one_mod_block")} <= set(TOP2_CASES)
assert all((T, fam) in TOP4_CASES for T in T_TOP4 for fam in FAMILIES[:3]) and (16, "multiple") in TOP4_CASES


class Setup:
    """one (E, top-k) stack pair in every resident form, and the oracle's results by (family, T)"""

    def __init__(self, E, topk, seed):
        from autoawq_amd.modules.fused import moe

        self.E, self.topk = E, topk
        w1, w2 = gemm_stacks(E, H, I, G, seed=seed)
        self.host = tuple(dict(qweight=s.qweight.numpy(), qzeros=s.qzeros.numpy(), scales=s.scales.numpy()) for s in (w1, w2))

        def device_pair():
            out = []
            for src in (w1, w2):
                s = Stack()
                s.qweight, s.qzeros, s.scales, s.group_size = src.qweight.cuda(), src.qzeros.cuda(), src.scales.cuda(), G
                out.append(s)
            return out
        self.plain = device_pair()
        self.twins = device_pair()
        t1, t2 = moe.build_decode_twins(*self.twins)
        assert t1 is not None and t2 is not None
        self.single = moe.build_single_copy(*self.plain)
        self.want = {}

    def logits(self, fam, T):
        return block_logits(self.E, self.topk, fam, T)

    def x(self, T):
        return torch.randn((T, H), generator=torch.Generator().manual_seed(T)).half()

    def reference(self, oracle, fam, T):
        """(want float64 [T, H], rms, ids) -- computed once per case, never written"""
        key = (fam, T)
        if key not in self.want:
            lg = self.logits(fam, T)
            want, ids, wt = oracle.moe_forward(self.x(T).numpy(), lg, self.host[0], self.host[1], self.topk, G)
            mr.check_route(lg, self.topk, True, wt, ids, f"oracle.moe_forward {fam} T{T}")  # the oracle routes as the reference does
            w64 = want.astype(np.float64)
            w64.setflags(write=False)
            self.want[key] = (w64, float(np.sqrt((w64 ** 2).mean())), ids)
        return self.want[key]


@pytest.fixture(scope="module")
def top2():
    return Setup(8, 2, seed=31)


@pytest.fixture(scope="module")
def top4():
    return Setup(4, 4, seed=43)


@pytest.fixture()
def moe(monkeypatch):
    """the dispatch module with single-copy mode handing over where two-copy mode does (the same kernels on the same integers)"""
    from autoawq_amd.modules.fused import moe as _moe

    monkeypatch.setattr(_moe, "ROWS_MAX_PAIRS_SINGLE", _moe.ROWS_MAX_PAIRS)
    assert (_moe.ROWS_MAX_PAIRS, _moe.DECODE_MAX_PAIRS, _moe.PREFILL_MIN_PAIRS) == (12, 64, 384), "the hand-overs moved: move the T values"
    return _moe


def expected_kernel(pairs, twins):
    if pairs >= 384:
        return "gemm_regb_grouped"
    return "gemv_rows_grouped" if twins and pairs <= 12 else "gemv_mfma_grouped"


def within(got, w64, rms):
    """(ok, max err / rms) under the block's tolerance 4e-3 |want| + 4e-3 rms (tests/test_gpu_moe_rows.py)"""
    y = got.cpu().numpy().astype(np.float64)
    err = np.abs(y - w64)
    return bool(np.isfinite(y).all() and (err <= 4e-3 * np.abs(w64) + 4e-3 * rms).all()), float(err.max() / rms)


def run_block_case(ops, oracle, moe, s, fam, T):
    lg = s.logits(fam, T)
    w64, rms, ids = s.reference(oracle, fam, T)
    if fam == "all_equal":
        assert (ids == np.arange(s.topk)[None]).all()
    if fam == "crowded" and s.E == 8:
        assert (ids == np.array(CROWD)[None]).all()
    if fam == "empties":
        assert set(np.unique(ids).tolist()) <= {0, s.E - 1}
    x, lgd = s.x(T).cuda(), torch.from_numpy(lg).cuda()
    pairs = T * s.topk
    out = {}
    for name, (a, b), twins in (("twins", s.twins, True), ("no twins", s.plain, False), ("single copy", s.single, True)):
        y = moe.apply_moe_weights(a, b, x, lgd, s.topk, True)
        assert ops.last_kernel() == expected_kernel(pairs, twins), (name, fam, T, ops.last_kernel())
        ok, r = within(y, w64, rms)
        print(f"moe block E{s.E} top-{s.topk} {fam} T{T} {name} [{ops.last_kernel()}]: max err / rms {r:.2e}")
        assert ok, (name, fam, T, r)
        out[name] = y
    assert torch.equal(out["single copy"], out["twins"]), (fam, T, "the single copy differs from two copies")
    return out


@pytest.mark.parametrize("T,fam", TOP2_CASES)
def test_moe_block_on_crafted_routes_at_every_hand_over(ops, oracle, moe, top2, T, fam):
    run_block_case(ops, oracle, moe, top2, fam, T)


@pytest.mark.parametrize("T,fam", TOP4_CASES)
def test_moe_block_top4_of_four_experts_on_crafted_routes(ops, oracle, moe, top4, T, fam):
    run_block_case(ops, oracle, moe, top4, fam, T)


@pytest.mark.parametrize("fam", ["crowded", "all_equal"])
@pytest.mark.parametrize("T", [6, 33])
@pytest.mark.parametrize("with_twins", [False, True])
def test_moe_expert_parallel_ranks_on_crafted_routes(ops, oracle, moe, top2, T, fam, with_twins):
    """world = 4: the fp32 sum of the ranks' parts, rounded once, against the oracle; a rank that owns no chosen expert returns
    exact zeros (crowded: experts 5 and 2, ranks 2 and 1; all_equal: experts 0 and 1, rank 0)"""
    from autoawq_amd import ep

    s, world = top2, 4
    w64, rms, ids = s.reference(oracle, fam, T)
    x, lgd = s.x(T).cuda(), torch.from_numpy(s.logits(fam, T)).cuda()
    total = torch.zeros((T, H), dtype=torch.float32, device="cuda")
    chosen = set(np.unique(ids).tolist())
    idle = 0
    for r in range(world):
        e0, e1 = ep.expert_bounds(s.E, r, world)
        a, b = ep.ExpertShard(s.plain[0], e0, e1), ep.ExpertShard(s.plain[1], e0, e1)
        if with_twins:
            moe.build_decode_twins(a, b)
        part = ep.apply_moe_weights_local(a, b, x, lgd, s.topk, True, e0)
        assert ops.last_kernel() == expected_kernel(T * s.topk, with_twins), (r, ops.last_kernel())
        if not chosen & set(range(e0, e1)):
            assert int(part.view(torch.int16).abs().max()) == 0, f"rank {r} owns no chosen expert and returns something"
            idle += 1
        total += part.float()
    assert idle == (3 if fam == "all_equal" else 2)
    ok, ratio = within(total.half(), w64, rms)
    print(f"moe expert-parallel world 4 {fam} T{T} twins={with_twins}: max err / rms {ratio:.2e}")
    assert ok, ratio


def test_moe_block_crowded_seven_tokens_captured_replays_bit_equal(ops, oracle, moe, top2):
    """T = 7 (14 pairs): the one-block route kernel with its alignment pass and the grouped block kernel inside a graph"""
    s, T = top2, 7
    w64, rms, _ = s.reference(oracle, "crowded", T)
    xs, ls = s.x(T).cuda(), torch.from_numpy(s.logits("crowded", T)).cuda()
    a, b = s.twins
    eager = moe.apply_moe_weights(a, b, xs, ls, s.topk, True)
    assert ops.last_kernel() == "gemv_mfma_grouped"
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        moe.apply_moe_weights(a, b, xs, ls, s.topk, True)
        st.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            out = moe.apply_moe_weights(a, b, xs, ls, s.topk, True)
        gr.replay()
        st.synchronize()
    assert torch.equal(out, eager)
    ok, r = within(out, w64, rms)
    print(f"moe block crowded T7 captured: max err / rms {r:.2e}")
    assert ok, r
