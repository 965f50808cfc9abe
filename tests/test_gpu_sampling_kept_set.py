"""The kept set of csrc/sample.hip, pinned exactly at bin, block and sign boundaries (MI355X): the adversarial rows of
tests/sampling_cases.py -- thresholds at low byte 0x00 / 0xFF and mid-bin, the +-0 and subnormal crossing, bin 4 at -65504 over
-inf filler, a tie group of 300 in every chunk, the top-p bin above / between / in the top-k bin, T from 0.05 to 8192, rows of 3
and 4 blocks read through aligned and unaligned views -- each drawn 256 times in one launch and held to the fp64 restatement by
sampling_cases.check_draws: every draw by the rule of tests/test_gpu_sampling.py, and over the schedule the in- and out-witnesses
and the emitted set.  tests/test_sampling_cases_cpu.py proves that a threshold one value off fails that check.

SAMPLING_KEPT_RECORD=<file>: every case appends "case form in-witnesses out-witnesses worst-score-gap/TOL" (recorded, not asserted)."""
import os

import numpy as np
import pytest
import torch

import penalty_ref as pref
import sampling_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from autoawq_amd import _lib, ops as o

    _lib.lib()
    return o


def record(case, form, stats):
    path = os.environ.get("SAMPLING_KEPT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(f"{case} {form} {stats.get('in_witnesses', '-')} {stats.get('out_witnesses', '-')} {stats['worst_gap_over_tol']:.4f}\n")


def _launch_rows(case):
    """`rows` copies of the row on the device: contiguous, or the last position of a [rows, 2, V + 3] buffer whose rows start 4 or
    12 bytes past a 16-byte line (load8's scalar path in every block; NaN everywhere else: a read outside the row poisons it)"""
    row = torch.from_numpy(case.raw.copy())
    if not case.strided:
        return row.repeat(case.rows, 1).cuda()
    big = torch.full((case.rows, 2, case.V + 3), float("nan"), dtype=torch.float16)
    big[:, 1, :case.V] = row
    view = big.cuda()[:, :, :case.V]
    assert all((view[r, -1].data_ptr() % 16) in (4, 12) for r in (0, 1, case.rows - 1))
    return view


def _clean_workspace(ops, x, B, V):
    ws = ops._sample_workspace(x.device, ops.sample_workspace_bytes(B, V))
    return int(ws.count_nonzero()) == 0


@pytest.mark.parametrize("case", sc.CASES, ids=[c.name for c in sc.CASES])
def test_shared_form_keeps_the_designed_set(ops, case):
    x = _launch_rows(case)
    tokens = []
    for t in case.ts:
        tokens.append(ops.sample_tokens(x, do_sample=True, seed=case.seed, t=t, **case.params).cpu().numpy())
        assert _clean_workspace(ops, x, case.rows, case.V), t
    stats = sc.check_draws(case, np.array(tokens))
    record(case.name, "shared", stats)


@pytest.mark.parametrize("V", [sc.V_A, sc.V_B, sc.V_C])
def test_rows_form_holds_every_row_to_its_own_case(ops, V):
    """row r carries case r % n with that case's temperature / top_k / top_p, a seed and a token index of its own; every third row is
    greedy.  A threshold, a mass or a count left in the workspace by one row would show in its neighbour, whose thresholds differ."""
    cases = sc.cases_of(V)
    n = len(cases)
    B = 6 * n
    of = [cases[r % n] for r in range(B)]
    x = torch.from_numpy(np.stack([c.raw for c in of])).cuda()   # (V = 6151: every other row starts 2 bytes off a 4-byte line)
    sample = [r % 3 != 0 for r in range(B)]
    seed = [1000 + 17 * r for r in range(B)]
    t = [1 + r % 5 for r in range(B)]
    out = ops.sample_tokens_rows(x, do_sample=sample, temperature=[c.temperature for c in of], top_k=[c.top_k for c in of],
                                 top_p=[c.top_p for c in of], seed=seed, t=t).cpu().tolist()
    assert _clean_workspace(ops, x, B, V)
    worst = {}
    for r in range(B):
        gap = sc.check_draw(of[r], out[r], seed=seed[r], t=t[r], row=r, do_sample=sample[r])
        worst[of[r].name] = max(worst.get(of[r].name, 0.0), gap)
    assert {c.name for r, c in enumerate(of) if sample[r]} == {c.name for r, c in enumerate(of) if not sample[r]} == set(worst)
    for name, gap in worst.items():
        record(name, "rows", {"worst_gap_over_tol": gap})


@pytest.mark.parametrize("case", sc.PROC_CASES, ids=[c.name for c in sc.PROC_CASES])
def test_processors_keep_the_set_of_the_processed_row(ops, case):
    """repetition_penalty moving a seen candidate across the threshold and a high-byte edge (down by division, up by
    multiplication), and min_new_tokens hiding the row maximum: the set is the set of penalty_ref.process(row)"""
    x = _launch_rows(case)
    before = pref.bitmap([case.seen] * case.rows, case.V)
    tokens = []
    for t in case.ts:
        hist = torch.from_numpy(before.copy()).cuda()
        out = ops.sample_tokens(x, do_sample=True, seed=case.seed, t=t, eos_ids=case.eos, repetition_penalty=case.penalty,
                                min_new_tokens=case.min_new, history=hist, **case.params).cpu().numpy()
        assert _clean_workspace(ops, x, case.rows, case.V), t
        want = before.view(np.uint32) | pref.bitmap([[int(o)] for o in out], case.V).view(np.uint32)
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), want), t
        tokens.append(out)
    stats = sc.check_draws(case, np.array(tokens))
    record(case.name, "processors", stats)
