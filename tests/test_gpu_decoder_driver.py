"""GraphedDecoder's one driver (capture, look-up, replay, advance, generate loop) on the committed tiny-Llama checkpoint (MI355X,
"gemv" layout, batch 3, max_seq_len 64, buckets 12 / 24: the fixture of test_gpu_generate_rows.py).  Every mode of the decoder
in turn on ONE decoder -- which family each mode captures into, that no mode drops or fills another mode's graphs, and that the
word resets and stream fences leave every call's result what a fresh decoder returns; a ring reallocation; and the one input on
which the scalar call and the call with per-row arguments trim their result differently.  Every comparison is exact."""
import pytest
import torch

from test_checkpoint import ckpt, skeleton
from test_gpu_generate_rows import MIXED, _ids

pytestmark = pytest.mark.gpu
B, P = 3, 6
FAMILIES = ("graphs", "row_graphs", "gen_graphs", "row_gen_graphs", "proc_gen_graphs", "row_proc_gen_graphs", "rows_gen_graphs",
            "spec_graphs", "verify_graphs")


@pytest.fixture(scope="module")
def lms():
    """two fused models of the same checkpoint: the decoder under test lives on the first, the fresh ones on the second (decoders
    on one model share its caches)"""
    from autoawq_amd.checkpoint import load_quantized
    from autoawq_amd.fuser import fuse_llama

    return [fuse_llama(load_quantized(skeleton(), ckpt("gemv"), device="cuda")[0], max_seq_len=64) for _ in range(2)]


def _decoder(lm):
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    return GraphedDecoder(lm, batch=B, buckets=(12, 24))


def _keys(dec):
    return {f: sorted(getattr(dec, f)) for f in FAMILIES}


def _mask():
    mask = torch.ones((B, P), dtype=torch.int64)
    mask[1, :2] = 0
    mask[2, :1] = 0
    return mask


def _steps(dec):
    dec.prefill(_ids(P))
    return torch.stack([dec.step(_ids(1, shift=s)).clone() for s in (1, 2, 3)])


def _eos_rows(dec):
    V = int(dec.lm.model.vocab_size)
    return [[V - 1], [V - 2, 5], [V - 3]]


def _verify(dec):
    """verify + advance_rows from ragged positions 6 / 4 / 5, then one step at the per-row positions it leaves (the step is one
    call more than the sequence asked for lists: it puts a key into `row_graphs`, the one family no other call here fills)"""
    dec.prefill(_ids(P), attention_mask=_mask())
    a = dec.verify(_ids(2, shift=5)).clone()
    dec.advance_rows([1, 2, 1])
    return torch.cat([a, dec.step(_ids(1, shift=9))], dim=1)


# (name, the call, the families it adds keys to).  Prompts of 6 tokens and 8 new ones: the steps run at cache lengths 7 .. 13, in
# the buckets 12 and 24.  A speculative run of 8 tokens replays 7 times with the host's bound growing by T = 3: 12, 24 and 64.
BOTH = [(12, True), (24, True)]
CALLS = [
    ("step x3", _steps, {"graphs": [12]}),
    ("greedy", lambda d: d.generate(_ids(P), max_new_tokens=8), {"gen_graphs": BOTH}),
    ("sampling", lambda d: d.generate(_ids(P), max_new_tokens=8, do_sample=True, temperature=0.7, top_p=0.9, seed=1),
     {"gen_graphs": [(12, False), (12, True), (24, False), (24, True)]}),
    ("penalty", lambda d: d.generate(_ids(P), max_new_tokens=8, repetition_penalty=1.3), {"proc_gen_graphs": BOTH}),
    ("ragged", lambda d: d.generate(_ids(P), max_new_tokens=8, attention_mask=_mask()), {"row_gen_graphs": BOTH}),
    ("ragged penalty", lambda d: d.generate(_ids(P), max_new_tokens=8, attention_mask=_mask(), repetition_penalty=1.3),
     {"row_proc_gen_graphs": BOTH}),
    ("per-row", lambda d: d.generate(_ids(P, shift=1), eos_token_id=_eos_rows(d), **MIXED), {"rows_gen_graphs": [12, 24]}),
    ("extend", lambda d: d.generate(_ids(4, shift=7), max_new_tokens=4, extend=True), {}),
    ("draft", lambda d: d.generate(_ids(P), max_new_tokens=8, draft_tokens=2), {"spec_graphs": [(12, 3), (24, 3), (64, 3)]}),
    ("verify", _verify, {"verify_graphs": [(12, 2)], "row_graphs": [12]}),
    ("greedy again", lambda d: d.generate(_ids(P), max_new_tokens=8), {}),
]
CALL = {name: fn for name, fn, _ in CALLS}
SHARES_STATE_WITH = {"extend": "per-row"}  # the one call that continues another: the fresh decoder runs that one first


def test_interleaved_modes_on_one_decoder(lms):
    want = {}
    for name, fn, _ in CALLS:
        fresh = _decoder(lms[1])
        if name in SHARES_STATE_WITH:
            CALL[SHARES_STATE_WITH[name]](fresh)
        want[name] = fn(fresh).clone()
    dec = _decoder(lms[0])
    keys = {f: [] for f in FAMILIES}
    assert _keys(dec) == keys
    for name, fn, adds in CALLS:
        got = fn(dec)
        keys.update(adds)
        assert _keys(dec) == keys, name
        assert got.dtype == want[name].dtype and torch.equal(got, want[name]), name
    assert torch.equal(want["greedy again"], want["greedy"])


def test_ring_reallocation_drops_the_scalar_families_only(lms):
    dec = _decoder(lms[0])
    for name in ("step x3", "sampling", "penalty", "ragged", "per-row", "draft", "verify"):
        CALL[name](dec)
    short = dec.generate(_ids(P), max_new_tokens=8)
    others = {f: dict(getattr(dec, f)) for f in ("graphs", "row_graphs", "rows_gen_graphs", "spec_graphs", "verify_graphs")}
    assert all(others.values()) and dec.proc_gen_graphs and dec.row_gen_graphs and (12, False) in dec.gen_graphs
    words = dec._gen
    # 300 tokens: a ring above the 256-column minimum, and the window of 64 rolls (the steps pass through every bucket)
    out = dec.generate(_ids(P), max_new_tokens=300)
    assert out.shape == (B, P + 300) and dec.position < 64
    assert dec._gen is not words and dec._gen["ring"].shape[1] == 300
    keys = _keys(dec)
    assert keys["gen_graphs"] == [(12, True), (24, True), (64, True)]            # only what this call captured
    assert keys["row_gen_graphs"] == keys["proc_gen_graphs"] == keys["row_proc_gen_graphs"] == []
    for f, before in others.items():                                              # the other modes' graphs: the same objects
        now = getattr(dec, f)
        assert sorted(now) == sorted(before) and all(now[k] is before[k] for k in before), f
    # t is the 1-based index of the NEXT token (test_gpu_generate.py pins 31 after 30 tokens): 300 generated
    assert int(dec._gen["t"]) == 300 + 1
    assert torch.equal(out[:, :P + 8], short)


def _second_turn(dec, ids1, ids2, mask2, **kw):
    """turn 1 (3 greedy tokens), row 2 sent back to position 0 with nothing pending, turn 2 with extend=True and an all-zero mask
    for it: that row has nothing to process, starts finished and emits pads"""
    dec.generate(ids1, max_new_tokens=3)
    dec.reset_rows([2])
    return dec.generate(ids2, attention_mask=mask2, extend=True, check_every=4, **kw)[:, ids2.shape[1]:].cpu()


def test_trim_with_an_idle_row_differs_between_scalar_and_per_row_arguments(lms):
    """Every live row finishes by its third token, the host sees `done` at its first look (check_every = 4), and the idle row's
    pad is not an EOS id.  The scalar call trims by each row's first EOS hit in the ring: the idle row has none, counts as the
    full width, and the result keeps the 4 columns at which `done` was seen.  The same request as per-row lists trims by the
    rows' real tokens (0 for the idle row): to the longest live row.  Widths recorded on the commit before the drivers were merged:
    4 and 3."""
    dec = _decoder(lms[0])
    ids1, ids2 = _ids(P), _ids(4, shift=7)
    mask2 = torch.ones((B, 4), dtype=torch.int64)
    mask2[2] = 0
    free = _second_turn(dec, ids1, ids2, mask2, max_new_tokens=8, pad_token_id=63)
    assert free.shape[1] == 8
    eos = sorted({int(free[0, 2]), int(free[1, 2])})         # the third token of each live row's greedy continuation
    pad = next(v for v in (63, 62, 61) if v not in eos)
    live = [min(i + 1 for i, t in enumerate(free[r].tolist()) if t in eos) for r in (0, 1)]
    scalar = _second_turn(dec, ids1, ids2, mask2, max_new_tokens=8, eos_token_id=eos, pad_token_id=pad)
    rows = _second_turn(dec, ids1, ids2, mask2, max_new_tokens=[8] * B, eos_token_id=[eos] * B, pad_token_id=pad)
    print(f"widths: scalar {scalar.shape[1]}, per-row arguments {rows.shape[1]}; live rows end at {live}")
    assert scalar.shape[1] == 4 and rows.shape[1] == max(live) == 3
    assert torch.equal(scalar[:, :3], rows) and (scalar[:, 3] == pad).all() and (rows[2] == pad).all()
    for r in (0, 1):
        assert rows[r].tolist() == free[r, :live[r]].tolist() + [pad] * (3 - live[r])
