"""The MoE routing kernels against the float64 reference of tests/moe_route_ref.py on crafted, decidable logits: awq_moe_route_kernel
(ids exactly -- ties go to the lowest index --, weights within the bound counted from its arithmetic, the block alignment whole,
globally and for a shard's experts, on both sides of the one-block / two-launch edge T = 8 | 9), awq_moe_sort_kernel (one expert
owning whole chunks, nothing but foreign ids, P = 1023 / 1025), the torch restatements on the device, and awq_silu_and_mul_kernel
past one pass of its grid."""
import numpy as np
import pytest
import torch

import moe_route_ref as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from autoawq_amd import _lib, ops as _ops

    _lib.lib()  # fails loudly if the extension is missing
    return _ops


def _np(t):
    return t.cpu().numpy()


def _route(ops, lg, k, renorm, block, e0=0, nl=None):
    return ops.moe_route(torch.from_numpy(lg).cuda(), k, renorm, block, first_expert=e0, num_local=nl)


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("T,E,k", mr.ROUTE_SHAPES)
def test_moe_route_ids_weights_and_alignment_vs_fp64_reference(ops, T, E, k, renorm):
    worst, n = {}, 0
    for block in mr.ROUTE_BLOCKS:
        for fam, lg in mr.cases(T, E, k, seed=T + E, block=block):
            assert mr.decidable(lg), fam
            what = f"{fam} T{T} E{E} k{k} renorm={renorm} block{block}"
            w, ids, s_ids, e_ids, npad = _route(ops, lg, k, renorm, block)
            worst[fam] = max(worst.get(fam, 0.0), mr.check_route(lg, k, renorm, _np(w), _np(ids), what))
            if block > 0:
                mr.check_alignment(_np(ids), E, block, _np(s_ids), _np(e_ids), _np(npad))
            else:
                assert s_ids is None and e_ids is None and npad is None
            n += 1
    print(f"moe_route T{T} E{E} k{k} renorm={renorm}: {n} cases, every row's ids equal; max err / bound",
          {f: round(r, 3) for f, r in worst.items()})


@pytest.mark.parametrize("T", [8, 9])
@pytest.mark.parametrize("E,k,e0,nl", mr.LOCAL_FORMS)
def test_moe_route_local_form_places_the_owned_pairs_and_leaves_the_routing_alone(ops, E, k, e0, nl, T):
    n = 0
    for block in (8, 16):
        for fam, lg in mr.cases(T, E, k, seed=T + E, block=block, e0=e0, nl=nl):
            assert mr.decidable(lg), fam
            what = f"{fam} T{T} E{E} k{k} block{block} experts {e0}+{nl}"
            gw, gids = _route(ops, lg, k, True, block)[:2]
            w, ids, s_ids, e_ids, npad = _route(ops, lg, k, True, block, e0, nl)
            assert torch.equal(ids, gids) and torch.equal(w.view(torch.int32), gw.view(torch.int32)), what
            mr.check_route(lg, k, True, _np(w), _np(ids), what)
            mr.check_alignment(_np(ids), E, block, _np(s_ids), _np(e_ids), _np(npad), e0=e0, nl=nl)
            n += 1
    assert n >= 16


@pytest.mark.parametrize("T,E,k,block", [(8, 64, 8, 8), (9, 64, 8, 8), (130, 16, 4, 16), (37, 8, 2, 0)])
def test_moe_route_is_bitwise_reproducible(ops, T, E, k, block):
    """(the counts are LDS atomics: their order may differ from call to call, nothing that is stored may)"""
    for fam, lg in mr.cases(T, E, k, seed=3, block=block, families=("ties", "crowded", "one_mod_block")):
        assert mr.decidable(lg), fam
        a, b = _route(ops, lg, k, True, block), _route(ops, lg, k, True, block)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)), fam


def _sort_cases():
    for E in (1, 8, 64):
        for P in (1, 1023, 1024, 1025, 2049):
            yield np.full(P, 63 if E == 64 else 0, np.int32), E, "one expert"
        foreign = np.where(np.arange(1500) % 2 == 0, -1, E + 3).astype(np.int32)
        yield foreign, E, "foreign"
        alt = np.where(np.arange(2049) % 2 == 0, np.arange(2049) % E, -1).astype(np.int32)
        alt[3::4] = E + 3
        yield alt, E, "alternating"


def test_moe_sort_whole_chunks_of_one_expert_foreign_ids_and_chunk_edges(ops):
    for ids, E, kind in _sort_cases():
        order, seg = ops.moe_sort_pairs(torch.from_numpy(ids).cuda().view(-1, 1), E)
        mr.check_sort(ids, E, _np(order), _np(seg))
        if kind == "foreign":
            assert not _np(seg).any()
    # ids as the route kernel writes them: every token on the same two experts, 700 tokens = two chunks
    lg = mr.build("crowded", 700, 8, 2, 1)
    assert mr.decidable(lg)
    ids = _route(ops, lg, 2, True, 0)[1]
    mr.check_route(lg, 2, True, _np(_route(ops, lg, 2, True, 0)[0]), _np(ids), "crowded T700")
    order, seg = ops.moe_sort_pairs(ids, 8)
    mr.check_sort(_np(ids), 8, _np(order), _np(seg))
    assert int((_np(seg)[1:] - _np(seg)[:-1] > 0).sum()) == 2


@pytest.mark.parametrize("T,E,k,block", [(9, 8, 2, 8), (130, 16, 4, 16)])
def test_torch_alignment_paths_on_the_device(ops, T, E, k, block):
    from autoawq_amd import ep

    half = (E + 1) // 2
    for fam, lg in mr.cases(T, E, k, seed=T, block=block):
        assert mr.decidable(lg), fam
        ids = mr.route_ref(lg, k, True)[1]
        dev = torch.from_numpy(ids).cuda()
        s, e, n = ops.moe_align_block_size(dev, block, E)
        mr.check_alignment(ids, E, block, _np(s), _np(e), _np(n))
        for e0, nl in ((0, half), (half, E - half), (E - 1, 1)):
            s, e, n, owned = ep.local_routing(dev, e0, nl, block)
            assert np.array_equal(_np(owned), (ids >= e0) & (ids < e0 + nl))
            mr.check_alignment(ids, E, block, _np(s), _np(e), _np(n), e0=e0, nl=nl, parked=True)


@pytest.mark.parametrize("rows,D", [(586, 14336), (1, 8), (37, 1408)])
def test_silu_and_mul_within_the_derived_bound_past_one_grid_pass(ops, rows, D):
    """586 x 14336 / 8 = 1,050,112 chunks of 8: more than the 4096 x 256 one pass of the grid covers, the grid-stride loop runs
    (every Mixtral-shape prefill is there)"""
    gu = mr.silu_input(rows, D, seed=4)
    got = _np(ops.silu_and_mul(torch.from_numpy(gu).cuda()))
    r = mr.check_silu(gu, got, f"silu_and_mul {rows} x {D}")
    print(f"silu_and_mul {rows} x {D}: max err / bound {r:.3f}")
