"""Prefill at per-row positions in GraphedDecoder (extend, reset_rows, generate(extend=True)) on the committed tiny-Llama
checkpoints: a prompt prefilled in two calls, a finished row's slot refilled while its neighbour goes on, and a second turn of a
conversation, each against this project's own one-shot prefill.  TOL is the checkpoint-logit tolerance of
test_gpu_spec_generate.py (2e-2 of the logit range)."""
import numpy as np
import pytest
import torch

from test_gpu_spec_generate import TOL, _decoder, _left_padded, _prompts

pytestmark = pytest.mark.gpu
PAD = 63


def _np(x):
    return x.double().cpu().numpy()


def _last(logits, mask):
    last = mask.shape[1] - 1 - mask.flip(1).argmax(1)
    return logits[torch.arange(logits.shape[0]), last]


_WHOLE = {}


def _whole(version, kw):
    """one prefill of the whole prompts (5 / 9 / 12 tokens, left-padded) and the step after it: the reference of the two-call test,
    computed once per (checkpoint, cache type)"""
    key = (version, tuple(sorted(kw.items())))
    if key not in _WHOLE:
        prompts = _prompts([5, 9, 12])
        ids, mask = _left_padded(prompts)
        dec = _decoder(version, 3, **kw)
        logits = _np(dec.prefill(ids, attention_mask=mask))
        nxt = torch.tensor([[7], [21], [40]])
        step = _np(dec.step(nxt.cuda())[:, 0])
        _WHOLE[key] = (prompts, logits, nxt, step)
    return _WHOLE[key]


@pytest.mark.parametrize("version", ["gemv", "gemm"])
@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_two_calls_equal_one(version, kv):
    """prefill of the first 2 / 9 / 7 tokens, then extend with the rest (row 1 brings nothing): the logits of every real column and
    of the step that follows are those of one prefill of the whole prompts.  The cache rows of the row without tokens are
    bit-identical before and after the extend."""
    kw = {} if kv == "fp16" else {"kv_cache_dtype": "fp8"}
    prompts, want, nxt, want_step = _whole(version, kw)
    lengths, split = [5, 9, 12], [2, 9, 7]
    S = max(lengths)
    rng = np.abs(want).max()
    dec = _decoder(version, 3, **kw)
    ids1, mask1 = _left_padded([p[:c] for p, c in zip(prompts, split)])
    got1 = _np(dec.prefill(ids1, attention_mask=mask1))
    assert dec.positions == split
    # the second call right-padded: a layout of its own
    W = max(n - c for n, c in zip(lengths, split))
    ids2 = torch.full((3, W), PAD, dtype=torch.int64)
    mask2 = torch.zeros((3, W), dtype=torch.int64)
    for b, (p, c) in enumerate(zip(prompts, split)):
        ids2[b, :len(p) - c] = p[c:]
        mask2[b, :len(p) - c] = 1
    assert mask2[1].sum() == 0
    caches = [b.attn.cache for b in dec.blocks]
    before = [(c.k[1, :9].clone(), c.v[1, :9].clone()) + ((c.k_scale[1, :9].clone(), c.v_scale[1, :9].clone()) if kv == "fp8" else ())
              for c in caches]
    got2 = _np(dec.extend(ids2.cuda(), attention_mask=mask2.cuda()))
    assert dec.positions == lengths and got2.shape == (3, W, want.shape[-1])
    for c, old in zip(caches, before):
        now = (c.k[1, :9], c.v[1, :9]) + ((c.k_scale[1, :9], c.v_scale[1, :9]) if kv == "fp8" else ())
        for a, b_ in zip(now, old):
            assert torch.equal(a.view(torch.uint8) if a.dtype != torch.float32 else a.view(torch.int32),
                               b_.view(torch.uint8) if b_.dtype != torch.float32 else b_.view(torch.int32))
    worst = 0.0
    for b, (n, c) in enumerate(zip(lengths, split)):
        whole = want[b, S - n:]                                     # the row's n real columns
        both = np.concatenate([got1[b, ids1.shape[1] - c:], got2[b, :n - c]])
        assert both.shape == whole.shape
        worst = max(worst, np.abs(both - whole).max() / rng)
        assert np.abs(both - whole).max() <= TOL * rng, b
    step = _np(dec.step(nxt.cuda())[:, 0])
    assert dec.positions == [n + 1 for n in lengths]
    assert np.abs(step - want_step).max() <= TOL * np.abs(want_step).max()
    print(f"{version} {kv}: worst logit difference {worst:.2e} of the range, step {np.abs(step - want_step).max() / np.abs(want_step).max():.2e}")


def test_extend_from_shared_mode_and_without_a_mask():
    """no mask: every row brings S tokens; from shared mode every row stands at `position`"""
    prompts = _prompts([10, 10])
    ids = torch.stack(prompts).cuda()
    dec = _decoder("gemv", 2)
    want = _np(dec.prefill(ids))
    dec = _decoder("gemv", 2)
    a = _np(dec.prefill(ids[:, :4]))
    assert dec.positions is None and dec.position == 4
    b = _np(dec.extend(ids[:, 4:]))
    assert dec.positions == [10, 10]
    assert np.abs(np.concatenate([a, b], 1) - want).max() <= TOL * np.abs(want).max()
    assert dec.extend(ids[:, :0]).shape == (2, 0, want.shape[-1]) and dec.positions == [10, 10]


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_refill_a_finished_slot(kv):
    """after some decode steps row 1 is reset and takes a new prompt while row 0 keeps its cache: row 0's next step is that of a run
    without the refill, row 1's logits those of a fresh decoder prefilled with the new prompt in row 1"""
    kw = {} if kv == "fp16" else {"kv_cache_dtype": "fp8"}
    first = _prompts([8, 6])
    ids, mask = _left_padded(first)
    toks = torch.tensor([[3, 5], [17, 9], [30, 41]])                 # three decode steps, any tokens
    nxt = torch.tensor([[12], [25]])
    new_prompt = _prompts([11])[0].flip(0)                            # 11 tokens that differ from what row 1 held

    def start():
        dec = _decoder("gemv", 2, **kw)
        dec.prefill(ids, attention_mask=mask)
        for t in toks:
            dec.step(t.view(2, 1).cuda())
        return dec

    plain = start()
    assert plain.positions == [11, 9]
    want0 = _np(plain.step(nxt.cuda())[0, 0])
    fresh = _decoder("gemv", 2, **kw)                                 # same batch size, the new prompt alone in row 1
    ids_f, mask_f = _left_padded([first[0][:1], new_prompt])
    want1 = _np(fresh.prefill(ids_f, attention_mask=mask_f)[1])
    want1_step = _np(fresh.step(nxt.cuda())[1, 0])

    dec = start()
    dec.reset_rows([1])
    assert dec.positions == [11, 0]
    ids_r = torch.full((2, 11), PAD, dtype=torch.int64)
    ids_r[1] = new_prompt
    mask_r = torch.zeros((2, 11), dtype=torch.int64)
    mask_r[1] = 1
    got1 = _np(dec.extend(ids_r.cuda(), attention_mask=mask_r.cuda())[1])
    assert dec.positions == [11, 11]
    assert np.abs(got1 - want1).max() <= TOL * np.abs(want1).max()
    step = _np(dec.step(nxt.cuda())[:, 0])
    assert np.abs(step[0] - want0).max() <= TOL * np.abs(want0).max()
    assert np.abs(step[1] - want1_step).max() <= TOL * np.abs(want1_step).max()
    with pytest.raises(ValueError):
        dec.reset_rows([2])


def _teacher_forced_rows(version, convo, emitted, B):
    """convo[b]: the whole conversation of row b (a list of ids); emitted[b]: the indices into it of the tokens generate chose.
    One fresh prefill of the conversations: every chosen token must be the argmax of the logits at the position before it wherever
    their top-2 margin exceeds TOL x range (the rule of test_gpu_spec_generate._teacher_forced).  Returns the share left out."""
    ids, mask = _left_padded([torch.tensor(c) for c in convo])
    dec = _decoder(version, B)
    logits = _np(dec.prefill(ids, attention_mask=mask))
    S = ids.shape[1]
    skipped = total = 0
    for b in range(B):
        off = S - len(convo[b])
        for i in emitted[b]:
            lg = logits[b, off + i - 1]
            top = np.sort(lg)[-2:]
            total += 1
            if top[1] - top[0] > TOL * np.abs(lg).max():
                assert int(np.argmax(lg)) == convo[b][i], (b, i)
            else:
                skipped += 1
    return skipped / max(total, 1)


@pytest.mark.parametrize("version", ["gemv", "gemm"])
def test_two_turns(version):
    """generate(turn 1) then generate(turn 2, extend=True), greedy, ragged rows, one row finishing early in turn 1: the conversation
    -- prompt 1, reply 1 up to its EOS, prompt 2, reply 2 -- fed whole to a fresh prefill gives every generated token as that
    position's argmax.  A row with neither new tokens nor a pending token returns pads only."""
    B, n1, n2 = 3, 8, 6
    p1 = _prompts([6, 9, 4])
    ids1, mask1 = _left_padded(p1)
    dec = _decoder(version, B)
    free = dec.generate(ids1, max_new_tokens=n1, attention_mask=mask1).cpu()[:, ids1.shape[1]:]
    # an EOS id that ends row 1 early and that row 0 never emits (so the call runs its full length)
    eos = next((int(t) for t in free[1, :4] if int(t) not in free[0].tolist() and int(t) != PAD), None)
    assert eos is not None, (free.tolist(), "row 1's first tokens all occur in row 0: pick other prompts")
    out1 = dec.generate(ids1, max_new_tokens=n1, attention_mask=mask1, eos_token_id=eos, pad_token_id=PAD).cpu()
    new1 = out1[:, ids1.shape[1]:]
    reply1 = []
    for b in range(B):
        row = new1[b].tolist()
        reply1.append(row[:row.index(eos) + 1] if eos in row else row)
    assert len(reply1[1]) <= 4 and len(reply1[0]) == n1 == new1.shape[1]
    n_cols = new1.shape[1]
    assert dec.tail["cache_rows"] == [len(p) + min(len(r), n_cols - 1) for p, r in zip(p1, reply1)]
    assert dec.tail["pending"] == [r[-1] if len(r) == n_cols else None for r in reply1]
    # turn 2: rows 0 and 1 bring tokens, row 2 only its pending token (or nothing at all, if it finished)
    p2 = [_prompts([5])[0].flip(0).tolist(), _prompts([3, 12])[1].tolist()[7:], []]
    W = max(len(p) for p in p2)
    ids2 = torch.full((B, W), PAD, dtype=torch.int64)
    mask2 = torch.zeros((B, W), dtype=torch.int64)
    for b, p in enumerate(p2):
        if p:
            ids2[b, W - len(p):] = torch.tensor(p)
            mask2[b, W - len(p):] = 1
    pending2 = dec.tail["pending"][2]
    out2 = dec.generate(ids2.cuda(), max_new_tokens=n2, attention_mask=mask2.cuda(), eos_token_id=eos, pad_token_id=PAD,
                        extend=True).cpu()
    assert torch.equal(out2[:, :W], ids2)
    new2 = out2[:, W:]
    convo, emitted = [], []
    for b in range(B):
        row = new2[b].tolist()
        reply2 = row[:row.index(eos) + 1] if eos in row else row
        if b == 2 and pending2 is None:
            assert all(t == PAD for t in row)
            reply2 = []
        c = p1[b].tolist() + reply1[b] + p2[b] + reply2
        convo.append(c)
        at1 = len(p1[b])
        at2 = at1 + len(reply1[b]) + len(p2[b])
        emitted.append(list(range(at1, at1 + len(reply1[b]))) + list(range(at2, at2 + len(reply2))))
    share = _teacher_forced_rows(version, convo, emitted, B)
    print(f"{version}: two turns, margin rule left out {share:.3f}; replies {[len(r) for r in reply1]} then {new2.shape[1]} columns")
    assert share <= 0.5   # (a property of the tiny model's logits, not of the code: at least half of the tokens are really checked)
    # a third call where one row has nothing at all to process: only pads for it
    idle = [b for b in range(B) if dec.tail["pending"][b] is None]
    if idle:
        b = idle[0]
        ids3 = torch.full((B, 2), 5, dtype=torch.int64)
        mask3 = torch.ones((B, 2), dtype=torch.int64)
        mask3[b] = 0
        rows_before = list(dec.tail["cache_rows"])
        out3 = dec.generate(ids3.cuda(), max_new_tokens=3, attention_mask=mask3.cuda(), pad_token_id=PAD, extend=True).cpu()
        assert (out3[b, 2:] == PAD).all() and dec.tail["cache_rows"][b] == rows_before[b] and dec.tail["pending"][b] is None


def test_a_row_with_nothing_to_process_emits_pads():
    """deterministic form of the idle row: EOS = a row's first greedy token, so that row finishes on token 1 of turn 1, and feeds
    its EOS (n > 1): no pending token; with an all-zero mask in turn 2 it starts finished"""
    ids = torch.stack(_prompts([7, 7])).cuda()
    dec = _decoder("gemv", 2)
    free = dec.generate(ids, max_new_tokens=3).cpu()[:, 7:]
    eos = int(free[0, 0])
    if int(free[1, 0]) == eos:
        pytest.fail("both rows start with the same token: pick other prompts")
    dec.generate(ids, max_new_tokens=4, eos_token_id=eos, pad_token_id=PAD)
    assert dec.tail["pending"][0] is None and dec.tail["cache_rows"][0] == 8
    ids2 = torch.tensor([[PAD, PAD], [4, 8]])
    mask2 = torch.tensor([[0, 0], [1, 1]])
    out = dec.generate(ids2.cuda(), max_new_tokens=4, attention_mask=mask2.cuda(), eos_token_id=eos, pad_token_id=PAD,
                       extend=True).cpu()
    assert out[0].tolist() == [PAD, PAD] + [PAD] * (out.shape[1] - 2)
    assert dec.tail["cache_rows"][0] == 8 and dec.tail["pending"][0] is None
    assert (out[1, 2:] != PAD).any()


def test_window_and_refusals():
    prompts = _prompts([10, 10])
    ids = torch.stack(prompts).cuda()
    dec = _decoder("gemv", 2, max_seq_len=64)
    dec.prefill(ids)
    long = torch.zeros((2, 54), dtype=torch.int64).cuda()
    mask = torch.ones((2, 54), dtype=torch.int64)
    mask[1, 50:] = 0
    logits = dec.extend(long, attention_mask=mask.cuda())            # row 0 ends exactly at max_seq_len
    assert dec.positions == [64, 60] and bool(torch.isfinite(logits[0]).all())
    launched = []
    dec.lm.extend = lambda *a, **k: launched.append(1)                # any launch past this point is a failure
    with pytest.raises(ValueError, match="window"):
        dec.extend(long[:, :5], attention_mask=torch.tensor([[0] * 5, [1] * 5]).cuda())   # 60 + 5 > 64
    with pytest.raises(ValueError, match="window"):
        dec.extend(long[:, :1])                                       # row 0 is full
    assert not launched and dec.positions == [64, 60]
    del dec.lm.extend
    with pytest.raises(ValueError, match="draft_tokens"):
        dec.generate(ids, max_new_tokens=4, draft_tokens=3, extend=True)
    with pytest.raises(ValueError):
        dec.extend(ids, attention_mask=torch.tensor([[1, 0, 1] + [0] * 7] * 2))
    with pytest.raises(ValueError):
        dec.extend(ids[:1])


def test_penalty_history_is_kept_across_turns():
    """repetition_penalty != 1 with extend=True: the bitmap of turn 1 (prompt and reply) stays and the new ids are added"""
    ids = torch.stack(_prompts([6, 6])).cuda()
    dec = _decoder("gemv", 2)
    out1 = dec.generate(ids, max_new_tokens=4, repetition_penalty=1.3).cpu()
    ids2 = torch.tensor([[50, 51], [52, 53]])
    dec.generate(ids2.cuda(), max_new_tokens=3, repetition_penalty=1.3, extend=True)
    hist = dec._gen["history"].cpu()
    for b in range(2):
        for t in out1[b].tolist() + ids2[b].tolist():
            assert (int(hist[b, t // 32]) >> (t % 32)) & 1, (b, t)
