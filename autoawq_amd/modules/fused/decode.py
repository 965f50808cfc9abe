"""GraphedDecoder: one decode step = one hipGraph replay, for a fused model built by autoawq_amd.fuser (round 4).

The reference decodes by calling the fused model once per token from `generate` (awq/modules/fused/model.py:60-109,
examples/benchmark.py:55-87): every step re-issues ~160 launches from Python.  On MI355X a 7B decode step is ~1.2 ms of GPU
time in ~160 launches of 3-10 us each; launching them from the host costs more than running them.  So a step is captured
ONCE and replayed:

  * the positions live in two device words (start position, cache length) that the captured step itself advances, so one
    graph serves every token (QuantAttentionFused.use_device_positions);
  * a launch inside a graph has a FIXED grid, but the best attention launch depends on the context length: a 32-way split of
    the cache with a merge kernel behind it is right at 4k tokens and costs 14 us per layer at 64.  The decoder therefore keeps
    one graph per LENGTH BUCKET (256, 1024, 4096, ... cache rows): the host knows the position (it drives the loop), picks the
    bucket, and the attention launch inside that graph is sized for the bucket's bound (one split and no merge launch up to
    256 rows); within a bucket the kernel deals the rows that exist to its splits from the device-side length;
  * the token ids and the logits are static buffers (`step` copies the ids in, returns the logits tensor of the graph);
  * a step that would run past the cache window forgets the oldest StepPlan.ROLL positions first (the reference's policy,
    awq/utils/fused_utils.py:14-25), eagerly, between two replays.

    dec = GraphedDecoder(fused_lm, batch=1)
    logits = dec.prefill(prompt_ids)          # eager, any length
    for _ in range(n):
        logits = dec.step(next_ids)           # [batch, 1, vocab]; valid until the next step

Every mode below goes through ONE driver.  A graph lives in a family -- a dict keyed by the bucket bound, and by whatever else is
baked into the graph -- and is made on first use: `_graph(family, key, ...)` is the one get-or-capture, `_capture` the one capture
skeleton (warm-up outside the capture, capture on the decoder's stream, the caller's stream fenced on both sides), `_replay` the
one fenced replay.  `_advance` is the one token step behind `step`, `replay` and `generate`: roll a full window, pick the bound,
pick family and key, replay, advance the host's position(s).  Shared and per-row mode differ there in the roll, the bound and
the advance alone.  `_first_logits` is what every `generate` does up to token 1's logits, and `_generate_loop` the one loop
behind the scalar call and the call with per-row arguments.  The families, what selects them and what their graphs hold:

    graphs[bound]                           row_graphs[bound]              step / replay                     the step
    gen_graphs[(bound, greedy)]             row_gen_graphs[...]            generate                          step + sampler
    proc_gen_graphs[(bound, greedy)]        row_proc_gen_graphs[...]       ... repetition_penalty /          step + sampler with the
                                                                           min_new_tokens                    logit processors
                                            rows_gen_graphs[bound]         generate, per-row arguments       step + rows sampler
                                            spec_graphs[(bound, T)]        generate(draft_tokens=T - 1)      verify step + argmax +
                                                                                                             accept + draft
                                            spec_sample_graphs[(bound, T)] ... draft_accept="sampler"        verify step + slots
                                                                                                             sampler + accept + draft
                                            verify_graphs[(bound, T)]      verify                            verify step
    lp_gen_graphs[(bound, (greedy, proc))]  row_lp_gen_graphs[...]         generate(logprobs=True)           step + sampler + log-prob
                                            row_lp_gen_graphs[(bound,      ... with per-row arguments        step + rows sampler +
                                                               "rows")]                                      log-prob
    (left: one shared position, the words `pos` / `len`; right: per-row positions, `pos_rows` / `len_rows`)

The graphs bake in the addresses of the device words their sampler reads, so a family lives as long as its words: `_gen_state`
drops the four scalar generation families when it reallocates (a longer ring, another vocabulary), its per-row form drops
`rows_gen_graphs`, `_spec_state(T)` the speculative graphs of that T; the log-prob graphs go with the state whose sampler they hold.

Token generation (`generate`): the same step, then the sampler (csrc/sample.hip) writing the next ids straight into the step's
input buffer, a ring of generated tokens and the per-row finished flags.  The host only picks buckets, rolls the window and looks
at the flags every `check_every` tokens.

    out = dec.generate(prompt_ids, max_new_tokens=64, do_sample=True, top_p=0.9, seed=1)   # [batch, prompt + n] int64

Prompts of different lengths come as one padded batch with an `attention_mask` (transformers' convention; modules/fused/
ragged.py).  Every row then has its own position: `pos_rows` / `len_rows` hold one word per row, the per-row families read them
through the *_rows kernels, the host keeps one position per row (`positions`), picks the bucket from the largest and rolls a
row's window on its own when that row alone would run past it.  No mask, or an all-ones mask, takes the shared words and graphs.

    out = dec.generate(ids, attention_mask=mask, max_new_tokens=64)   # left-padded ids: transformers' layout

repetition_penalty / min_new_tokens (transformers' logit processors) run inside the sampler's passes, reading a per-row bitmap of
the ids seen so far that the sampler itself extends.  With both at their defaults the sampler is launched without them: the
kernels that read neither.

Per-row arguments (a sequence of `batch` values for a sampling argument, a list of lists for eos_token_id): every row is a request
of its own.  One family, the sampler's rows form with the processors always attached, device words of its own (`_gen_rows`).

Speculative decoding (`generate(draft_tokens=K)`, `verify` / `advance_rows`): one pass over the weights for T = K + 1 tokens per
row.  A graph of `spec_graphs` runs the model on tok [B, T] at the per-row positions (rope + append of T rows,
csrc/verify_attn.hip), takes the greedy argmax of every slot with the sampler, keeps the longest run of drafts the model agrees
with (awq_spec_accept: ring, history, positions and finished flags advance on the device by what was accepted) and writes the next
step's drafts by prompt lookup in the row's own history (awq_ngram_draft).  Rejected drafts leave cache rows at and above the
row's new position; the next step's append overwrites them, nothing is rolled back.  The host only bounds the positions between
checks, and its loop stays its own (`_generate_spec`): a replay emits a variable number of tokens.  `verify_graphs` is the same
step without the two integer kernels, for callers with drafts of their own.  draft_tokens=0 (the default) creates none of this.

    out = dec.generate(ids, max_new_tokens=128, draft_tokens=3, draft_ngram=3)   # the text of the plain greedy run
    dec.last_spec                                                                 # {"replays": r, "new_tokens": [n_b ...]}

draft_accept="sampler": the same loop with sampling and the logit processors.  The sampler's token is a deterministic function of the
logits, (seed, token index, row) and the processors' state, so the graph (family `spec_sample_graphs`, device words of its own:
`_spec_sample`) asks the sampler's slots form (awq_sample_tokens_slots) which token the plain sampler would emit at every slot's
token index given the drafts before it, and awq_spec_accept_ex keeps a draft exactly when it is that token -- for a point-mass draft
the acceptance probability p(draft) of rejection sampling -- and extends the penalty history by what was emitted.  The text is the
plain sampled run's, token for token.  The default draft_accept="argmax" runs the graphs and launches above, unchanged.

    out = dec.generate(ids, max_new_tokens=128, do_sample=True, temperature=0.7, seed=1, draft_tokens=3, draft_accept="sampler")

Prefill at per-row positions (`extend`, `reset_rows`, `generate(extend=True)`): eager, no graph family.  `extend` appends row b's
tokens at ITS position (rope + append with per-row counts, then csrc/prefill_attn.hip's rows form) and leaves the decoder in
per-row mode; a row with an all-zero mask is untouched.  `reset_rows` sends rows back to position 0 and keeps the others: a
finished row's slot takes a new prompt while its neighbours go on.  `generate` records what it left in the caches per row (`tail`:
modules/fused/ragged.py, generate_tail_rows), and a following `generate(extend=True)` continues from there instead of restarting.

    out1 = dec.generate(turn1, max_new_tokens=64, eos_token_id=eos)
    out2 = dec.generate(turn2, max_new_tokens=64, eos_token_id=eos, extend=True)   # turn 1 is not prefilled again

Log-probabilities (`generate(logprobs=True)`, `score`): csrc/logprob.hip, one block per row, under the model's own distribution
(no temperature, top-k / top-p or logit processor).  In `generate` the launch is recorded right behind the sampler: it reads the
step's logits and the ids the sampler has just written into `tok`, and appends to a ring of its own (`lp` [B, cap] fp32 at the
per-row slot word `lp_slot`) beside the sampler's words -- no host round trip per token.  Such graphs live in families of their
own; a call without `logprobs` finds, captures and replays exactly the graphs it did before, and allocates none of this.
`score` is one prefill and one launch over the [B, S, V] logits with shifted labels.

    out = dec.generate(ids, max_new_tokens=64, logprobs=True)
    dec.last_logprobs                      # fp32 [batch, n]: aligned with out[:, prompt:], 0.0 past a row's real tokens
    lp = dec.score(ids, attention_mask)    # fp32 [batch, S]: log p(ids[b, s] | the row's real tokens before it)
"""
import torch

from ... import ops
from ..._lib import AwqHipError
from .model import StepPlan
from .ragged import generate_tail_rows, mask_runs, mask_runs_extend, pack_ids, unpack_rows


class GraphedDecoder:
    BUCKETS = (256, 1024, 4096, 16384, 65536, 262144)

    def __init__(self, lm, batch=1, buckets=None):
        self.lm = lm
        self.blocks = list(lm.model.blocks)
        self.device = self.blocks[0].device if hasattr(self.blocks[0], "device") else next(lm.parameters()).device
        self.device = torch.device(self.device)
        if self.device.type != "cuda":
            raise RuntimeError("GraphedDecoder needs the model on a HIP device")
        self.batch = int(batch)
        # A captured step bakes every HOST-side length into the graph.  Only the native decode path of QuantAttentionFused (head_dim
        # 128 with 1, 2, 4 or 8 query heads per KV head: csrc/decoder.hip) reads its positions from the device words; other head
        # shapes slice the cache with the host's start_pos and would attend over the capture-time row count on every replay
        # (ADVICE r04): refuse them here instead of returning silently wrong logits.
        for i, b in enumerate(self.blocks):
            a = b.attn
            if a.head_dim != 128 or a.n_kv_groups not in (1, 2, 4, 8):
                raise NotImplementedError(f"GraphedDecoder: block {i} has head_dim {a.head_dim} and {a.n_kv_groups} query heads per KV head; "
                                          "only the native decode attention (head_dim 128; 1, 2, 4 or 8 heads per KV head) takes its "
                                          "positions from the device -- decode this model eagerly")
        self.max_seq_len = min(b.attn.max_seq_len for b in self.blocks)
        bounds = sorted(set(min(int(b), self.max_seq_len) for b in (buckets or self.BUCKETS)))
        if bounds[-1] < self.max_seq_len:
            bounds.append(self.max_seq_len)
        self.bounds = bounds
        with torch.inference_mode(False):  # persistent buffers written in place from any context: never inference tensors
            self.pos = torch.zeros(1, dtype=torch.int32, device=self.device)   # start position of the step
            self.len = torch.ones(1, dtype=torch.int32, device=self.device)    # cache rows after its append
            self.tok = torch.zeros((self.batch, 1), dtype=torch.int64, device=self.device)
            self.pos_rows = torch.zeros(self.batch, dtype=torch.int32, device=self.device)  # per-row mode: start position of
            self.len_rows = torch.ones(self.batch, dtype=torch.int32, device=self.device)   # each row, its cache rows after the append
        self.stream = torch.cuda.Stream(device=self.device)
        self.graphs = {}  # bucket bound -> (graph, logits)
        self.gen_graphs = {}  # (bucket bound, greedy) -> (graph, logits): step + sampler (generate)
        self.row_graphs = {}  # per-row mode (attention_mask): bucket bound -> (graph, logits), reading pos_rows / len_rows
        self.row_gen_graphs = {}  # per-row mode: (bucket bound, greedy) -> (graph, logits)
        self.proc_gen_graphs = {}  # with the logit processors (repetition_penalty / min_new_tokens): keyed as gen_graphs
        self.row_proc_gen_graphs = {}  # ... and as row_gen_graphs
        self._gen = None  # generate's device words (allocated by its first call)
        self.rows_gen_graphs = {}  # generate with per-row arguments: bucket bound -> (graph, logits): per-row positions + rows sampler
        self._gen_rows = None      # ... and its device words (one AwqSampleParams / AwqSampleProc / t / max_new per row)
        self._history_of_last = None  # the history the last `generate` kept up to date (None: it ran without the processors)
        self.spec_graphs = {}    # speculative decoding: (bucket bound, T) -> (graph, logits): verify step + argmax + accept + draft
        self.verify_graphs = {}  # (bucket bound, T) -> (graph, logits): the verify step alone (`verify`)
        self._spec = {}          # T -> the device words of the speculative path (allocated by its first use)
        self.spec_sample_graphs = {}  # draft_accept="sampler": (bucket bound, T) -> (graph, logits): verify step + slots sampler + accept + draft
        self._spec_sample = {}   # ... and its device words per T: those of `_spec` (addresses of their own) + params / proc / history per row
        self._verify_T = None    # tokens appended by the last `verify`, until `advance_rows`
        self.last_spec = None
        self.lp_gen_graphs = {}      # generate(logprobs=True): (bucket bound, (greedy, proc)) -> (graph, logits): step + sampler + log-prob
        self.row_lp_gen_graphs = {}  # ... at per-row positions; (bucket bound, "rows"): the call with per-row arguments
        self.last_logprobs = None    # fp32 [batch, n] of the last generate(logprobs=True); None after a call without
        self.tail = None         # what the last plain `generate` left per row: {"cache_rows": [...], "pending": [...]} (generate_tail)
        self.position = 0
        self.positions = None  # per-row mode: the host's position of every row (None: one shared position)
        for b in self.blocks:
            b.attn._resize_cache(self.batch)

    # ---- bookkeeping ------------------------------------------------------------------------------------------------
    def _sync_host_state(self):
        # (per-row mode: the largest position -- the host-side bookkeeping of the blocks then never rolls the shared window,
        #  the rows that would run past it have been rolled one by one before)
        if self.positions is not None:
            self.position = max(self.positions)
        for b in self.blocks:
            b.attn.start_pos = self.position
        self.lm.model.last_forward_num_tokens = self.position

    def seek(self, position):
        """Declare that `position` cache rows are valid (benchmarks and tests that fill the caches themselves).  Like every
        other move of the positions from outside `generate`, it drops `tail`."""
        if not 0 <= position <= self.max_seq_len:  # (== max_seq_len: a full window -- the next step rolls it first)
            raise ValueError(f"position {position} outside the cache window {self.max_seq_len}")
        self.positions = None
        self.tail = None
        self.position = int(position)
        self.pos.fill_(self.position)
        self.len.fill_(self.position + 1)
        self._sync_host_state()

    def seek_rows(self, positions):
        """Per-row mode: declare that row b has positions[b] valid cache rows.  Later steps use the per-row graphs."""
        positions = [int(p) for p in positions]
        if len(positions) != self.batch:
            raise ValueError(f"seek_rows: {len(positions)} positions for a batch of {self.batch}")
        if not all(0 <= p <= self.max_seq_len for p in positions):
            raise ValueError(f"seek_rows: positions {positions} outside the cache window {self.max_seq_len}")
        self.positions = positions
        self.tail = None
        p = torch.tensor(positions, dtype=torch.int32)
        self.pos_rows.copy_(p)
        self.len_rows.copy_(p + 1)
        self._sync_host_state()

    def bucket(self, rows):
        for b in self.bounds:
            if rows <= b:
                return b
        return self.bounds[-1]

    # ---- prefill: eager (any number of tokens; the reference's own path) ----------------------------------------------
    def _ragged(self, input_ids, attention_mask):
        """(starts, lengths) of the mask's runs, or None when there is no mask or every row is full (the shared path)"""
        if attention_mask is None:
            return None
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch:
            raise ValueError(f"input_ids must be [{self.batch}, prompt] with an attention_mask, got {tuple(input_ids.shape)}")
        starts, lengths = mask_runs(attention_mask, input_ids.shape, max_len=self.max_seq_len)
        if all(n == input_ids.shape[1] for n in lengths):
            return None
        return starts, lengths

    def _prefill_eager(self, input_ids):
        for b in self.blocks:
            b.attn.use_device_positions(None, None)
            b.attn.start_pos = 0
        self.lm.model.last_forward_num_tokens = 0
        return self.lm(input_ids.to(self.device))

    @torch.inference_mode()
    def prefill(self, input_ids, attention_mask=None):
        """input_ids [B, S] -> logits [B, S, vocab], eager.  attention_mask [B, S] of 0 / 1 (transformers' convention, each row's
        ones one contiguous run: left or right padding): row b's L_b real tokens get positions 0 .. L_b - 1 and the decoder
        switches to per-row positions.  The logits come back in the caller's layout; the values at pad columns are
        unspecified.  No mask, or an all-ones mask, is exactly the unmasked call."""
        input_ids = input_ids.to(self.device)
        ragged = self._ragged(input_ids, attention_mask)
        if ragged is None:
            logits = self._prefill_eager(input_ids)
            self.seek(self.blocks[0].attn.start_pos)
            return logits
        starts, lengths = ragged
        logits = self._prefill_eager(pack_ids(input_ids, starts, lengths))  # [B, max L_b, V]: row b's tokens at 0 .. L_b - 1
        self.seek_rows(lengths)
        return unpack_rows(logits, starts, lengths, input_ids.shape[1])

    # ---- prefill at per-row positions: eager ---------------------------------------------------------------------------------
    def _row_positions(self):
        return list(self.positions) if self.positions is not None else [self.position] * self.batch

    def _extend_packed(self, packed, base, lengths):
        """packed [B, W] ids, row b's lengths[b] tokens at columns 0 ..: appended at positions base[b] ..  Returns the logits
        [B, W, V] and leaves the decoder in per-row mode at base[b] + lengths[b]."""
        ends = [p + n for p, n in zip(base, lengths)]
        if max(ends) > self.max_seq_len:  # before any launch
            raise ValueError(f"extend: positions {base} + {lengths} tokens run past the cache window {self.max_seq_len} "
                             "(extend never rolls the window)")
        pos = torch.tensor(base, dtype=torch.int32).to(self.device)
        cnt = torch.tensor(lengths, dtype=torch.int32).to(self.device)
        logits = self.lm.extend(packed, pos, cnt, max(ends))
        self.seek_rows(ends)
        return logits

    @torch.inference_mode()
    def extend(self, input_ids, attention_mask=None):
        """input_ids [B, S] -> logits [B, S, vocab], eager: `prefill` that continues.  Row b's L_b >= 0 real tokens (attention_mask as
        in `prefill`, but a row may be all zeros; no mask: L_b = S) take positions p_b .. p_b + L_b - 1, p_b the row's current
        position (shared mode: `position` for every row); what the row has cached below p_b stays and is attended to.  A row
        with L_b = 0 is untouched.  Afterwards the decoder is in per-row mode at p_b + L_b.  The logits come back in the
        caller's layout; the values at pad columns are unspecified.  p_b + L_b > max_seq_len raises ValueError: extend never
        rolls the window."""
        input_ids = input_ids.to(self.device)
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch:
            raise ValueError(f"input_ids must be [{self.batch}, tokens], got {tuple(input_ids.shape)}")
        S = input_ids.shape[1]
        if attention_mask is None:
            starts, lengths = [0] * self.batch, [S] * self.batch
        else:
            starts, lengths = mask_runs_extend(attention_mask, input_ids.shape)
        base = self._row_positions()
        if S == 0:
            self.seek_rows(base)
            return torch.zeros((self.batch, 0, int(self.lm.model.vocab_size)), dtype=torch.float16, device=self.device)
        # (a row without tokens is packed as if it had one: its count stays 0, so nothing of it is appended or attended)
        logits = self._extend_packed(pack_ids(input_ids, starts, [max(n, 1) for n in lengths]), base, lengths)
        return unpack_rows(logits, starts, lengths, S)

    def reset_rows(self, rows):
        """The rows listed go back to position 0 and the others keep theirs (per-row mode from here on).  Nothing is cleared:
        cache rows at and above a row's position are dead by construction.  A following `extend` with a mask that is zero in the
        other rows puts a new prompt into these slots."""
        rows = [int(r) for r in rows]
        if not all(0 <= r < self.batch for r in rows):
            raise ValueError(f"reset_rows: rows {rows} outside the batch of {self.batch}")
        base = self._row_positions()
        for r in rows:
            base[r] = 0
        tail = self.tail
        self.seek_rows(base)
        if tail is not None:  # the other rows still owe their last token
            for r in rows:
                tail["cache_rows"][r], tail["pending"][r] = 0, None
            self.tail = tail

    def _extend_turn(self, input_ids, attention_mask):
        """generate(extend=True) up to token 1's logits: every row goes back to what the last generate left in its cache (`tail`),
        the token that call emitted last and never fed is put in front of the row's new tokens, and the lot is extended.
        Returns (logits [B, 1, V] at every row's last new position, the rows with nothing to process)."""
        B, S = input_ids.shape
        if attention_mask is None:
            starts, lengths = [0] * B, [S] * B
        else:
            starts, lengths = mask_runs_extend(attention_mask, input_ids.shape)
        tail = self.tail if self.tail is not None else {"cache_rows": self._row_positions(), "pending": [None] * B}
        rows = []
        for b in range(B):
            new = input_ids[b, starts[b]:starts[b] + lengths[b]].long()
            if tail["pending"][b] is not None:
                new = torch.cat([torch.tensor([tail["pending"][b]], dtype=torch.int64, device=new.device), new])
            rows.append(new)
        counts = [int(r.numel()) for r in rows]
        idle = [b for b, n in enumerate(counts) if n == 0]
        width = max(max(counts), 1)
        packed = torch.zeros((B, width), dtype=torch.int64, device=self.device)
        for b, r in enumerate(rows):
            packed[b, :counts[b]] = r
        logits = self._extend_packed(packed, list(tail["cache_rows"]), counts)
        last = torch.tensor([max(n - 1, 0) for n in counts], dtype=torch.int64, device=self.device)
        return logits[torch.arange(B, device=self.device), last].unsqueeze(1).contiguous(), idle

    def _first_logits(self, input_ids, attention_mask, extend=False, per_row=False):
        """What every generate path does up to token 1's logits: `_extend_turn`, or prefill and -- for prompts of different
        lengths -- the gather of each row's last real column.  Returns (logits, the rows with nothing to process).  Unpadded
        input leaves the positions shared unless per_row: then every row gets a position of its own, the one they share."""
        if extend:
            return self._extend_turn(input_ids, attention_mask)
        ragged = self._ragged(input_ids, attention_mask)
        logits = self.prefill(input_ids, attention_mask if ragged is not None else None)
        if ragged is not None:  # the first token of row b comes from its column start_b + L_b - 1
            last = torch.tensor([s + n - 1 for s, n in zip(*ragged)], dtype=torch.int64, device=self.device)
            logits = logits[torch.arange(self.batch, device=self.device), last].unsqueeze(1).contiguous()
        elif per_row:
            self.seek_rows([self.position] * self.batch)
        return logits, []

    # ---- one driver: capture, look-up, replay, advance -----------------------------------------------------------------------
    @torch.inference_mode()
    def _capture(self, bound, rows, body, advance):
        """The one capture skeleton -> (graph, logits).  body(capturing) runs the model on the decoder's static ids and returns
        the logits: once eagerly (the warm-up: it appends cache rows at the current positions, which the first replay writes
        again with the real tokens, and builds every lazily cached buffer OUTSIDE the capture), once recorded.  What moves the
        decoder's words belongs under `capturing` alone.  rows: the blocks read pos_rows / len_rows.  advance: the recorded step
        also moves its position words on by one, and they are restored from clones afterwards."""
        pos, ln = (self.pos_rows, self.len_rows) if rows else (self.pos, self.len)
        for b in self.blocks:
            b.attn.use_device_positions(pos, ln, per_row=rows, bound=bound)
        keep = (pos.clone(), ln.clone()) if advance else None
        caller = torch.cuda.current_stream(self.device)  # (taken BEFORE entering the decoder's stream: the ids were copied on it)
        with torch.cuda.stream(self.stream):
            self.stream.wait_stream(caller)
            body(False)
            self._sync_host_state()  # (the model's eager step moved the blocks' host bookkeeping; a verify step did not: a no-op there)
            self.stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=self.stream):
                logits = body(True)
                if advance:
                    pos.add_(1)
                    ln.add_(1)
            self.stream.synchronize()
            if advance:
                pos.copy_(keep[0])
                ln.copy_(keep[1])
        caller.wait_stream(self.stream)
        self._sync_host_state()
        return graph, logits

    def _step_body(self, capturing, sample):
        logits = self.lm(self.tok)
        if capturing and sample is not None:
            sample(logits)
        return logits

    def _spec_body(self, capturing, st, full):
        """the verify step; full: + the slots' tokens (argmax, or the slots sampler on the words of draft_accept="sampler"), and --
        recorded only, they move the decoder's words -- accept and draft"""
        logits = self.lm.verify(st["tok"])
        if full:
            self._spec_tail(st, logits)
            if capturing:
                more = {"history": st["history"], "vocab": st["vocab"]} if "history" in st else {}
                ops.spec_accept(st["params"], st["tok"], st["pred"], st["hist"], st["n_hist"], st["cnt"], st["ring"],
                                st["finished"], self.pos_rows, self.len_rows, status=st["status"], steps=st["steps"], **more)
                ops.ngram_draft(st["params"], st["tok"], st["hist"], st["n_hist"])
        return logits

    def _graph(self, family, key, bound, rows, advance, body, *args):
        """The one get-or-capture: family[key] = (graph, logits), captured on first use from body(capturing, *args) under the
        bucket bound `bound`."""
        entry = family.get(key)
        if entry is None:
            entry = family[key] = self._capture(bound, rows, lambda capturing: body(capturing, *args), advance)
        return entry

    def _replay(self, graph):
        """one replay on the decoder's stream, fenced against the caller's work on both sides"""
        caller = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(caller)   # the ids were copied on the caller's stream
        with torch.cuda.stream(self.stream):
            graph.replay()
        caller.wait_stream(self.stream)   # ... and the caller reads the logits

    def _roll_rows(self):
        """Per-row mode: every row that alone would run past the window forgets its oldest StepPlan.ROLL positions, as
        roll_kv_n_steps does for a row decoded alone; the other rows keep their contents."""
        over = [r for r, p in enumerate(self.positions) if p + 1 > self.max_seq_len]
        if not over:
            return
        for r in over:
            n = max(0, min(StepPlan.ROLL, self.positions[r], self.max_seq_len))
            for b in self.blocks:
                b.attn.cache.roll_rows([r], n)
            self.positions[r] -= n
        self.seek_rows(self.positions)

    def _advance(self, shared, per_row, tag=None, sample=None):
        """One token, for `step`, `replay` and the generate loop: roll a full window, pick (or capture) the bucket's graph, replay
        it, advance the position(s) on the host as the graph did on the device.  shared / per_row: the family of the mode at one
        shared position and at per-row positions (shared None: the mode runs at per-row positions only); tag: what follows the
        bound in its keys (None: the bound alone); sample: the sampler call recorded behind the step (None: the step graphs).
        Shared and per-row mode differ in the roll, the bound and the host's advance."""
        self.tail = None  # (generate states it again when it is done)
        rows = self.positions is not None
        if rows:
            self._roll_rows()
            bound, family = self.bucket(max(self.positions) + 1), per_row
        else:
            if self.position + 1 > self.max_seq_len:  # past the window: forget the oldest positions (eagerly)
                live = [b.attn.cache.roll_kv_n_steps(self.position, n=StepPlan.ROLL) for b in self.blocks][0]
                self.seek(live)
            bound, family = self.bucket(self.position + 1), shared
        key = bound if tag is None else (bound, tag)
        entry = family.get(key)  # (once per token: the hit costs one dict look-up, `_graph` is entered on a miss alone)
        if entry is None:
            entry = self._graph(family, key, bound, rows, True, self._step_body, sample)
        graph, logits = entry
        self._replay(graph)
        if rows:
            self.positions = [p + 1 for p in self.positions]
        else:
            self.position += 1
        self._sync_host_state()
        return logits

    @torch.inference_mode()
    def step(self, token_ids):
        """token_ids [batch, 1] (or [batch]): the tokens at the current position.  Returns the logits [batch, 1, vocab] -- the
        graph's static output buffer, overwritten by the next step."""
        self.tok.copy_(token_ids.reshape(self.batch, 1))
        return self._advance(self.graphs, self.row_graphs)

    @torch.inference_mode()
    def replay(self):
        """The current bucket's graph once more on the decoder's stream with the ids already in place (benchmarks: no host
        copies in the timed region).  Same roll / stream / host bookkeeping as `step`."""
        return self._advance(self.graphs, self.row_graphs)

    # ---- generation: sampler in the graph ---------------------------------------------------------------------------------
    def _gen_state(self, vocab, cap, per_row=False, logprobs=False):
        """The device words generate owns (per_row: of generate with per-row arguments -- params / proc / t hold one element per
        row, and max_new).  Their addresses are baked into the generation graphs: reallocated (and those graphs dropped) only when
        the vocabulary or the ring capacity has to grow.  logprobs: also lp (fp32 [B, ring capacity]: the log-probabilities of the
        generated tokens) and lp_slot (int32 [B]: the column each row writes next) -- added on the first call that asks for them,
        so the words and graphs of plain calls are untouched, and reallocated with the ring.  history: the ids seen per row (bit v % 32 of word v / 32), proc: struct
        AwqSampleProc -- the logit processors' state."""
        g = self._gen_rows if per_row else self._gen
        if g is None or g["vocab"] != vocab or g["ring"].shape[1] < cap:
            g = self._gen_alloc(vocab, cap, per_row)
        if logprobs and "lp" not in g:
            with torch.inference_mode(False):
                g["lp"] = torch.zeros((self.batch, g["ring"].shape[1]), dtype=torch.float32, device=self.device)
                g["lp_slot"] = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        return g

    def _gen_alloc(self, vocab, cap, per_row):
        with torch.inference_mode(False):
            dev, B = self.device, self.batch
            one = (B,) if per_row else ()  # one parameter word per row, or one for all
            g = {"vocab": vocab,
                 "params": torch.zeros(one + (64,), dtype=torch.uint8, device=dev),
                 "proc": torch.zeros(one + (16,), dtype=torch.uint8, device=dev),
                 "t": torch.ones(B if per_row else 1, dtype=torch.int32, device=dev),
                 "ring": torch.zeros((B, max(int(cap), 256)), dtype=torch.int32, device=dev),
                 "finished": torch.zeros(B, dtype=torch.int32, device=dev),
                 "status": torch.zeros((B + 31) // 32, dtype=torch.int32, device=dev),
                 "ws": torch.zeros(ops.sample_workspace_bytes(B, vocab), dtype=torch.uint8, device=dev),
                 "history": torch.zeros((B, ops.sample_history_words(vocab)), dtype=torch.int32, device=dev)}
            if per_row:
                g["max_new"] = torch.zeros(B, dtype=torch.int32, device=dev)
        if per_row:
            self.rows_gen_graphs = {}
            self.row_lp_gen_graphs = {k: v for k, v in self.row_lp_gen_graphs.items() if k[1] != "rows"}
            self._gen_rows = g
        else:
            self.lp_gen_graphs = {}
            self.row_lp_gen_graphs = {k: v for k, v in self.row_lp_gen_graphs.items() if k[1] == "rows"}
            self.gen_graphs = {}
            self.row_gen_graphs = {}
            self.proc_gen_graphs = {}
            self.row_proc_gen_graphs = {}
            self._gen = g
        return g

    def _sample(self, logits, g, per_row, greedy, proc):
        """the sampler on the words g, writing the next ids into the step's input buffer; per_row: g holds per-row words (the rows form)"""
        launch, more = (ops.sample_launch_rows, {"max_new": g["max_new"]}) if per_row else (ops.sample_launch, {})
        launch(logits, g["params"], g["t"], self.tok.view(-1), g["status"], g["ws"], ring=g["ring"], finished=g["finished"],
               greedy=greedy, proc=g["proc"] if proc else None, history=g["history"] if proc else None, **more)

    def _logprob(self, logits, g):
        """the log-probability of the ids the sampler has just written into the step's input buffer, appended to g's ring"""
        ops.token_logprobs_launch(logits, self.tok, g["lp"], slot=g["lp_slot"])

    def _check(self, g):
        st = g["status"].cpu()
        if bool(st.any()):
            bad = [r for r in range(self.batch) if (int(st[r // 32]) >> (r % 32)) & 1]
            raise AwqHipError(f"generate: rows {bad} produced NaN / +inf logits or kept no token")
        return bool(g["finished"].cpu().all())

    def _generate_loop(self, input_ids, logits, idle, extend, check_every, mode):
        """The one generate loop, from token 1's logits to the ids returned.  mode describes the call: g (its device words), words
        (name -> the CPU bytes this call puts into them), sample (the sampler call: eagerly for token 1, recorded behind the
        step), advance (`_advance`'s two families -- taken after `_gen_state`, which may replace them -- and its tag), eos /
        budgets (one list of EOS ids and one max_new_tokens per row), and per_row / proc / moved for the three places where the
        scalar call and the call with per-row arguments differ.  logprobs: g holds lp / lp_slot and `sample` ends with the
        log-prob launch; `last_logprobs` is set from them."""
        g, sample, eos_rows, budgets = mode["g"], mode["sample"], mode["eos"], mode["budgets"]
        shared, rows_family, tag = mode["advance"]
        # reset every decoder-owned device word, outside any capture; every token index restarts at 1
        for name, value in mode["words"].items():
            g[name].copy_(value)
        g["t"].fill_(1)
        g["ring"].zero_()
        g["finished"].zero_()
        if idle:  # nothing to process: the row starts finished and emits pads
            g["finished"][torch.tensor(idle, device=self.device)] = 1
        g["status"].zero_()
        if mode["logprobs"]:
            g["lp"].zero_()
            g["lp_slot"].zero_()
        # History carry-over under extend differs between the two calls, and stays so.
        if mode["per_row"]:
            # per-row arguments: the processors always run, and what moves along is the history the LAST generate kept up to
            # date, whichever words it lives in (none: the sampler knows this turn's ids only)
            prev = self._history_of_last
            if not extend or prev is None:
                g["history"].zero_()
            elif prev is not g["history"] and prev.shape == g["history"].shape:
                g["history"].copy_(prev)
            ops.sample_history(input_ids, g["vocab"], out=g["history"])
            self._history_of_last = g["history"]
        else:
            # scalars: the history is touched only when the processors are on; under extend it stays as it is in these words, or
            # comes from the words this call replaced (`moved`: reallocated for a longer ring, same vocabulary)
            self._history_of_last = g["history"] if mode["proc"] else None
            if mode["proc"]:
                if not extend:
                    g["history"].zero_()
                elif mode["moved"] is not None:
                    g["history"].copy_(mode["moved"])
                ops.sample_history(input_ids, g["vocab"], out=g["history"])
        sample(logits)  # token 1, eagerly, into self.tok
        n, n_max = 1, max(budgets)
        while n < n_max:
            if n % check_every == 0 and self._check(g):
                break
            self._advance(shared, rows_family, tag, sample)  # step on token n, sample token n + 1
            n += 1
        done = self._check(g)
        new = g["ring"][:, :n]
        # what this call leaves in the caches, for a following generate(extend=True).  n - 1 tokens were fed since token 1 was
        # sampled: counted back from where the rows stand now, a window roll in between is accounted for
        lengths = [p - (n - 1) for p in self._row_positions()]
        cache_rows, pending, real = generate_tail_rows(lengths, new.cpu().tolist(), eos_rows, budgets, n, idle=idle)
        self.tail = {"cache_rows": cache_rows, "pending": pending}
        lp = None
        if mode["logprobs"]:  # a row's slots past its real tokens (the pads after its end, every slot of an idle row) hold 0.0
            keep = torch.arange(n, device=self.device).view(1, -1) < torch.tensor(real, device=self.device).view(-1, 1)
            lp = torch.where(keep, g["lp"][:, :n], torch.zeros((), dtype=torch.float32, device=self.device))
        # The trim of all-pad columns differs between the two calls, and stays so.
        if done and mode["per_row"]:
            # per-row arguments: stop where the longest row ended, by the tail's count of real tokens (0 for an idle row)
            n = max(1, min(n, max(real)))
        elif done and eos_rows[0]:
            # scalars (HF stops at the step where the last row finished): only with EOS ids, and by each row's first EOS hit in the
            # ring -- an idle row whose pad is no EOS id has none, counts as n and keeps the result untrimmed
            hit = torch.zeros_like(new, dtype=torch.bool)
            for e in eos_rows[0]:
                hit |= new == e
            first = torch.where(hit.any(1), hit.int().argmax(1), torch.full_like(hit[:, 0], n, dtype=torch.int64))
            n = min(n, int(first.max()) + 1)
        self.last_logprobs = None if lp is None else lp[:, :n].contiguous()
        return torch.cat([input_ids.long(), new[:, :n].long()], dim=1)  # (rows past their end already hold their own pad)

    # ---- speculative decoding --------------------------------------------------------------------------------------------
    def _spec_check_model(self, T):
        from .model import MixtralModel

        if not 2 <= T <= 8:
            raise ValueError(f"a verify step takes 2 .. 8 tokens per row (draft_tokens 1 .. 7), got {T}")
        if self.batch * T > 1024:
            raise ValueError(f"batch * (draft_tokens + 1) = {self.batch * T} exceeds the sampler's 1024 rows")
        if any(b.attn.kv_cache_dtype == "fp8" for b in self.blocks):
            raise NotImplementedError('speculative decoding: kv_cache_dtype="fp8" is not supported (the verify attention reads '
                                      "fp16 caches)")
        if isinstance(self.lm.model, MixtralModel):
            raise NotImplementedError("speculative decoding: fuse_mixtral models are refused (the MoE block under a verify step "
                                      "is not covered by tests)")

    def _spec_state(self, T, vocab=None, ring_cap=0, hist_cap=0, sampler=False):
        """The device words of the speculative path for steps of T tokens; their addresses are baked into the graphs of that T,
        which are dropped when the words have to be reallocated (another vocabulary, a longer ring or history).  sampler: the
        words of draft_accept="sampler" -- the same set at addresses of its own, and the slots sampler's per-row params / proc /
        history; the greedy path's words and graphs are not touched."""
        store = self._spec_sample if sampler else self._spec
        st = store.get(T)
        if st is not None and (vocab is None or st["vocab"] == vocab) and st["ring"].shape[1] >= ring_cap and st["hist"].shape[1] >= hist_cap:
            return st
        if vocab is None:
            vocab = int(self.lm.model.vocab_size) if st is None else st["vocab"]
        B, dev = self.batch, self.device
        with torch.inference_mode(False):
            st = {"vocab": vocab,
                  "tok": torch.zeros((B, T), dtype=torch.int64, device=dev),
                  "pred": torch.zeros(B * T, dtype=torch.int64, device=dev),
                  "params": torch.zeros(48, dtype=torch.uint8, device=dev),         # struct AwqSpecParams
                  "argmax_params": ops.sample_params(do_sample=False).to(dev),      # the slots' argmax: greedy, no EOS ids
                  "t": torch.ones(1, dtype=torch.int32, device=dev),
                  "status": torch.zeros((B * T + 31) // 32, dtype=torch.int32, device=dev),
                  "ws": torch.zeros(ops.sample_workspace_bytes(B * T, vocab), dtype=torch.uint8, device=dev),
                  "hist": torch.zeros((B, max(int(hist_cap), 256)), dtype=torch.int32, device=dev),
                  "n_hist": torch.zeros(B, dtype=torch.int32, device=dev),
                  "cnt": torch.zeros(B, dtype=torch.int32, device=dev),
                  "ring": torch.zeros((B, max(int(ring_cap), 256)), dtype=torch.int32, device=dev),
                  "finished": torch.zeros(B, dtype=torch.int32, device=dev),
                  "steps": torch.zeros(B, dtype=torch.int32, device=dev)}
            if sampler:
                st.update({"sparams": torch.zeros((B, 64), dtype=torch.uint8, device=dev),   # struct AwqSampleParams [B]
                           "proc": torch.zeros((B, 16), dtype=torch.uint8, device=dev),      # struct AwqSampleProc [B]
                           "history": torch.zeros((B, ops.sample_history_words(vocab)), dtype=torch.int32, device=dev)})
        if sampler:
            self.spec_sample_graphs = {k: v for k, v in self.spec_sample_graphs.items() if k[1] != T}
        else:
            self.spec_graphs = {k: v for k, v in self.spec_graphs.items() if k[1] != T}
            self.verify_graphs = {k: v for k, v in self.verify_graphs.items() if k[1] != T}
        store[T] = st
        return st

    def _spec_tail(self, st, logits):
        """The token of each of the B * T slots.  Greedy: the argmax by the sampler itself (its tie and NaN / +inf rules), no ring,
        no flags, no EOS ids.  draft_accept="sampler": the slots form -- what the plain sampler would emit at the slot's token
        index after the drafts before it; it writes pred and status alone, so the warm-up may run it."""
        if "sparams" in st:
            ops.sample_launch_slots(logits, st["sparams"], st["cnt"], st["tok"], st["pred"], st["status"], st["ws"],
                                    finished=st["finished"], proc=st["proc"], history=st["history"])
            return
        ops.sample_launch(logits.view(-1, logits.shape[-1]), st["argmax_params"], st["t"], st["pred"], st["status"], st["ws"],
                          greedy=True)

    def _replay_spec(self, bound, T, full, sampler=False):
        family = self.spec_sample_graphs if sampler else self.spec_graphs if full else self.verify_graphs
        graph, logits = self._graph(family, (bound, T), bound, True, False, self._spec_body,
                                    (self._spec_sample if sampler else self._spec)[T], full)
        self._replay(graph)
        return logits

    @torch.inference_mode()
    def verify(self, token_ids):
        """token_ids [batch, T], T = 2 .. 8: row b's tokens at positions p_b .. p_b + T - 1 (its last token, then T - 1 drafts).
        Returns the logits [batch, T, vocab] -- slot j is what `step` would return after the first j + 1 of them; the graph's
        static buffer, overwritten by the next call.  T cache rows are appended per row and NOTHING advances: `advance_rows`
        then says how many of them each row keeps.  Switches the decoder to per-row positions."""
        token_ids = token_ids.to(self.device)
        if token_ids.dim() != 2 or token_ids.shape[0] != self.batch:
            raise ValueError(f"verify: token_ids must be [{self.batch}, T], got {tuple(token_ids.shape)}")
        T = int(token_ids.shape[1])
        self._spec_check_model(T)
        if self.positions is None:
            self.seek_rows([self.position] * self.batch)
        if max(self.positions) + T > self.max_seq_len:
            raise ValueError(f"verify: positions {self.positions} + {T} tokens run past the cache window {self.max_seq_len} "
                             "(no window roll inside a speculative step)")
        st = self._spec_state(T)
        st["tok"].copy_(token_ids)
        logits = self._replay_spec(self.bucket(max(self.positions) + T), T, full=False)
        self._verify_T = T
        return logits

    def advance_rows(self, counts):
        """After `verify`: row b keeps the first counts[b] of the T tokens it appended (1 <= counts[b] <= T); the rows of the
        others lie at and above its new position and are overwritten by the next step."""
        counts = [int(c) for c in counts]
        if self._verify_T is None:
            raise RuntimeError("advance_rows follows a verify call")
        if len(counts) != self.batch or not all(1 <= c <= self._verify_T for c in counts):
            raise ValueError(f"advance_rows: {self.batch} counts in 1 .. {self._verify_T} expected, got {counts}")
        self._verify_T = None
        self.seek_rows([p + c for p, c in zip(self.positions, counts)])

    def _generate_spec(self, input_ids, max_new_tokens, K, ngram, eos, pad_token_id, check_every, attention_mask, sampler=None):
        """The speculative run.  sampler: None (greedy: the slots' argmax), or the sampling arguments of draft_accept="sampler" --
        token 1 by the plain sampler with the processors, the slots by its slots form; everything else is shared."""
        T = K + 1
        self._spec_check_model(T)
        B, S = input_ids.shape
        ragged = self._ragged(input_ids, attention_mask)
        starts, lengths = ragged if ragged is not None else ([0] * B, [S] * B)
        if max(lengths) + max_new_tokens + T > self.max_seq_len:
            raise ValueError(f"speculative generate: prompt ({max(lengths)}) + max_new_tokens ({max_new_tokens}) + {T} step tokens "
                             f"exceed the cache window {self.max_seq_len} (no window roll inside a speculative run)")
        pad = int(pad_token_id) if pad_token_id is not None else (eos[0] if eos else 0)
        params = ops.spec_params(eos_ids=eos, pad=pad, max_new_tokens=max_new_tokens, ngram_max=ngram)
        # always per-row: equal positions diverge at the first step (unpadded: the shared position is every row's length)
        logits, _ = self._first_logits(input_ids, attention_mask, per_row=True)
        st = self._spec_state(T, logits.shape[-1], max_new_tokens, max(lengths) + max_new_tokens, sampler=sampler is not None)
        if sampler is None:
            first = ops.sample_tokens(logits, do_sample=False)  # token 1, eagerly (raises on NaN / +inf logits)
        else:
            # the plain path's start: the history holds input_ids as passed, token 1 is the plain sampler's at t = 1 (row b keys
            # its Philox counter, as request b keys the slots'), which also adds it to the history
            st["sparams"].copy_(ops.sample_params_rows(B, eos_ids=eos, pad=pad, **sampler["params"]))
            st["proc"].copy_(ops.sample_proc_params_rows(B, **sampler["proc"]))
            st["history"].zero_()
            ops.sample_history(input_ids, st["vocab"], out=st["history"])
            first = ops.sample_tokens(logits, t=1, eos_ids=eos, pad=pad, history=st["history"], **sampler["params"], **sampler["proc"])
        # reset the decoder-owned words outside any capture: prompt and token 1 into the history, token 1 into the ring
        n_hist = torch.tensor(lengths, dtype=torch.int64, device=self.device)
        st["params"].copy_(params)
        st["status"].zero_()
        st["ring"].zero_()
        st["hist"].zero_()
        st["hist"][:, :max(lengths)] = pack_ids(input_ids, starts, lengths).to(torch.int32)
        st["hist"].scatter_(1, n_hist.view(-1, 1), first.to(torch.int32).view(-1, 1))
        st["n_hist"].copy_((n_hist + 1).to(torch.int32))
        st["ring"][:, 0] = first.to(torch.int32)
        st["cnt"].fill_(1)
        st["steps"].zero_()
        hit = torch.zeros(B, dtype=torch.bool, device=self.device)
        for e in eos:
            hit |= first == e
        st["finished"].copy_((hit | (max_new_tokens <= 1)).to(torch.int32))
        ops.ngram_draft(st["params"], st["tok"], st["hist"], st["n_hist"])
        upper, replays = list(lengths), 0
        words = None
        for _ in range(max_new_tokens - 1):  # every replay emits at least one token per unfinished row: the budget ends the run
            if replays % check_every == 0:   # one copy: the flags, and the positions that make the host's bounds exact again
                words = torch.cat([st["finished"], self.pos_rows]).cpu().tolist()
                if all(words[:B]):
                    break
                upper = words[B:]
            self._replay_spec(self.bucket(min(max(upper) + T, self.max_seq_len)), T, full=True, sampler=sampler is not None)
            upper = [u + T for u in upper]
            replays += 1
        words = torch.cat([st["finished"], self.pos_rows, st["cnt"], st["steps"], st["status"]]).cpu().tolist()
        bad = sorted({r // T for r in range(B * T) if (words[4 * B + r // 32] >> (r % 32)) & 1})
        if bad:
            raise AwqHipError(f"generate: rows {bad} produced NaN / +inf logits" + (" or kept no token" if sampler is not None else ""))
        cnt = words[2 * B:3 * B]
        self.seek_rows(words[B:2 * B])
        # replays: those the slowest row needed (the host may have launched a few more before its next look at the flags)
        self.last_spec = {"replays": max(words[3 * B:4 * B]), "new_tokens": cnt, "launched": replays}
        n = max(cnt)
        new = st["ring"][:, :n].long()
        keep = torch.arange(n, device=self.device).view(1, -1) < torch.tensor(cnt, device=self.device).view(-1, 1)
        new = torch.where(keep, new, torch.full_like(new, pad))
        return torch.cat([input_ids.long(), new], dim=1)

    def _generate_rows(self, input_ids, args, eos_token_id, pad_token_id, check_every, attention_mask, extend, logprobs=False):
        """generate with per-row arguments (see `generate`): every check of the arguments comes before the first launch."""
        B = self.batch
        max_rows = []
        for r, m in enumerate(ops.per_row("max_new_tokens", args["max_new_tokens"], B)):
            if isinstance(m, bool) or int(m) != m or int(m) < 1:
                raise ValueError(f"row {r}: max_new_tokens must be an integer >= 1, got {m}")
            max_rows.append(int(m))
        if eos_token_id is None or isinstance(eos_token_id, int):
            eos_rows = [[] if eos_token_id is None else [int(eos_token_id)]] * B
        else:
            eos_rows = [[int(e) for e in row] for row in ops._eos_rows(eos_token_id, B)]
        params = ops.sample_params_rows(B, do_sample=args["do_sample"], temperature=args["temperature"], top_k=args["top_k"],
                                        top_p=args["top_p"], seed=args["seed"], eos_ids=eos_rows, pad=pad_token_id)
        proc_bytes = ops.sample_proc_params_rows(B, args["repetition_penalty"], args["min_new_tokens"])
        # the rows family reads per-row positions, and its sampler always runs the processors
        logits, idle = self._first_logits(input_ids, attention_mask, extend, per_row=True)
        g = self._gen_state(logits.shape[-1], max(max_rows), per_row=True, logprobs=logprobs)

        def sample(lg):
            self._sample(lg, g, True, False, True)
            if logprobs:
                self._logprob(lg, g)
        return self._generate_loop(input_ids, logits, idle, extend, check_every, {
            "g": g, "words": {"params": params, "proc": proc_bytes, "max_new": torch.tensor(max_rows, dtype=torch.int32)},
            "sample": sample, "advance": (None, self.row_lp_gen_graphs, "rows") if logprobs else (None, self.rows_gen_graphs, None),
            "eos": eos_rows, "budgets": max_rows, "per_row": True, "proc": True, "moved": None, "logprobs": logprobs})

    @torch.inference_mode()
    def generate(self, input_ids, max_new_tokens, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                 eos_token_id=None, pad_token_id=None, check_every=16, attention_mask=None, repetition_penalty=1.0,
                 min_new_tokens=0, draft_tokens=0, draft_ngram=3, extend=False, logprobs=False, draft_accept="argmax"):
        """input_ids [batch, prompt] -> [batch, prompt + n] int64 on the device, n <= max_new_tokens; rows that emitted an EOS id
        are padded with pad_token_id (default: the first EOS id) from then on, and the run stops once every row has (HF's
        `generate` semantics).  The prompt is prefilled eagerly and token 1 sampled eagerly from its last position; every later
        token is one replay of the bucket's generation graph.  The host reads the finished flags and the status word once
        every `check_every` tokens -- no host sync per token.  Sampling as ops.sample_tokens: temperature, top_k, top_p,
        Gumbel-max draw with Philox numbers keyed by (seed, token index, row).
        attention_mask [batch, prompt] (0 / 1, see `prefill`): prompts of different lengths; row b's first token is sampled
        from its logits at its last real position and every row then advances at its own position.  The result is still
        cat([input_ids, new], 1): for left-padded input, the layout transformers' `generate` returns.
        repetition_penalty (> 0, 1 = off) and min_new_tokens (>= 0, 0 = off): transformers' RepetitionPenaltyLogitsProcessor and
        MinNewTokensLengthLogitsProcessor, applied inside the sampler (ops.sample_tokens).  The penalty covers every id of
        input_ids as passed (pad columns included, as transformers' input_ids carry them) and every generated token (pads of
        finished rows included), also after a window roll has dropped their cache rows.
        draft_tokens = K in 1 .. 7 (0 = off): greedy speculative decoding by prompt lookup (transformers'
        `prompt_lookup_num_tokens`) -- every replay verifies K drafts found by matching the row's last draft_ngram .. 1 tokens
        earlier in its own text and emits 1 .. K + 1 tokens; the text is the plain greedy run's (up to ties the two launch shapes
        round differently).  `last_spec` then holds {"replays": those the slowest row needed, "new_tokens": per row, "launched"}.  With the default
        draft_accept="argmax" this is greedy only (do_sample with temperature > 0, repetition_penalty != 1 and min_new_tokens > 0
        raise ValueError).  An fp8 cache raises NotImplementedError, and there is no window roll: prompt + max_new_tokens + K + 1 <=
        max_seq_len for every row.
        draft_accept="sampler" (needs draft_tokens >= 1): speculative decoding with scalar do_sample, temperature, top_k, top_p,
        seed, repetition_penalty and min_new_tokens.  The sampler's token is a deterministic function of the logits, (seed, token
        index, row) and the processors' state, so every slot of a verify step asks which token the plain sampler would emit at its
        token index given the drafts before it (ops.sample_tokens_slots), and a draft is accepted exactly when it is that token --
        with probability p(draft), the acceptance probability of rejection sampling for a point-mass draft.  Row b's tokens are those
        of `generate` without draft_tokens and with the same arguments, except at positions where the two launch shapes round the
        logits differently.  Graphs and device words of its own (`spec_sample_graphs`); a call with "argmax" and a plain call run
        exactly the graphs they ran before.  Not with per-row arguments, extend=True or logprobs=True (ValueError), an fp8 cache or
        a fuse_mixtral model (NotImplementedError); any other value of draft_accept raises ValueError.
        extend=True: input_ids / attention_mask (a row may be all zeros) are APPENDED to each row's context instead of
        restarting it -- the next turn of a conversation.  Every row goes back to what the previous call left in its cache
        (`tail`: its prompt and the real tokens it was fed; the pads fed to a finished row are dropped), the last token that call
        emitted without feeding it comes first, then the new tokens, in one `extend`.  A row with neither starts finished and
        emits pads.  The repetition-penalty history is kept and extended by the new ids.  Not with draft_tokens (ValueError);
        the window is `extend`'s: no roll while the new tokens are appended.
        Per-row arguments: each of do_sample, temperature, top_k, top_p, seed, max_new_tokens, repetition_penalty and
        min_new_tokens also takes a sequence of `batch` values, and eos_token_id a list of lists (one per row; None: no EOS id):
        every row is a request of its own.  Such a call uses the sampler's rows form (ops.sample_tokens_rows) in one graph family
        of its own (`rows_gen_graphs`: per-row positions, processors attached); row r's tokens are those of the call with row r's
        values as scalars.  The loop runs to max(max_new_tokens); a row past its own limit is finished on the device and padded
        with its pad (pad_token_id, default the row's first EOS id), and n is the longest row's count.  With extend=True every
        row's token index restarts at 1.  Not with draft_tokens (ValueError).  All scalars: the path above, unchanged.
        logprobs=True: the result is unchanged and `last_logprobs` is set to fp32 [batch, n] on the device, aligned with the new
        columns of the result: the log-probability of each generated token under the model's OWN distribution (log-softmax of the
        raw logits: temperature, top_k / top_p, repetition_penalty and min_new_tokens are not applied -- what serving APIs return
        as `logprobs`).  A row's slots past its real tokens -- the pads after its EOS or its own max_new_tokens, every slot of an
        idle row -- hold 0.0.  The values are computed on the device by a launch recorded behind the sampler, in graph families of
        their own; a call without logprobs sets `last_logprobs` to None and runs exactly the graphs it ran before.  Not with
        draft_tokens (ValueError)."""
        input_ids = input_ids.to(self.device)
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch:
            raise ValueError(f"input_ids must be [{self.batch}, prompt], got {tuple(input_ids.shape)}")
        logprobs = bool(logprobs)
        if draft_accept not in ("argmax", "sampler"):
            raise ValueError(f'generate: draft_accept must be "argmax" or "sampler", got {draft_accept!r}')
        if draft_accept == "sampler" and not draft_tokens:
            raise ValueError('generate: draft_accept="sampler" needs draft_tokens >= 1 (it names how drafts are accepted)')
        if logprobs and draft_tokens:
            raise ValueError("generate: logprobs is not available with draft_tokens (a speculative step emits a variable number "
                             "of tokens per replay)")
        self.last_logprobs = None
        per_row = {"do_sample": do_sample, "temperature": temperature, "top_k": top_k, "top_p": top_p, "seed": seed,
                   "max_new_tokens": max_new_tokens, "repetition_penalty": repetition_penalty, "min_new_tokens": min_new_tokens}
        eos_per_row = (eos_token_id is not None and ops.is_seq(eos_token_id)
                       and any(e is None or ops.is_seq(e) for e in eos_token_id))
        if eos_per_row or any(ops.is_seq(v) for v in per_row.values()):
            if draft_tokens:
                raise ValueError("generate: draft_tokens does not take per-row arguments (speculative decoding is one greedy "
                                 "request per batch)")
            return self._generate_rows(input_ids, per_row, eos_token_id, pad_token_id, max(1, int(check_every)), attention_mask,
                                       extend, logprobs)
        max_new_tokens, check_every = int(max_new_tokens), max(1, int(check_every))
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id])
        if draft_tokens and extend:
            raise ValueError("generate(extend=True) does not take draft_tokens: the speculative path keeps no history across calls")
        if draft_tokens:
            if isinstance(draft_tokens, bool) or int(draft_tokens) != draft_tokens or not 1 <= int(draft_tokens) <= 7:
                raise ValueError(f"draft_tokens must be an integer in 0 .. 7, got {draft_tokens}")
            if draft_accept == "sampler":
                sampler = {"params": {"do_sample": do_sample, "temperature": temperature, "top_k": top_k, "top_p": top_p, "seed": seed},
                           "proc": {"repetition_penalty": repetition_penalty, "min_new_tokens": min_new_tokens}}
                ops.sample_params(eos_ids=eos, pad=pad_token_id, **sampler["params"])  # the checks of the values, before any launch
                ops.sample_proc_params(**sampler["proc"])
                return self._generate_spec(input_ids, max_new_tokens, int(draft_tokens), int(draft_ngram), eos, pad_token_id,
                                           check_every, attention_mask, sampler=sampler)
            if do_sample and float(temperature) > 0:
                raise ValueError("speculative decoding is greedy: do_sample with temperature > 0 needs rejection sampling")
            if float(repetition_penalty) != 1.0 or int(min_new_tokens) > 0:
                raise ValueError("speculative decoding does not run the logit processors (repetition_penalty, min_new_tokens)")
            return self._generate_spec(input_ids, max_new_tokens, int(draft_tokens), int(draft_ngram), eos, pad_token_id,
                                       check_every, attention_mask)
        params = ops.sample_params(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, eos_ids=eos,
                                   pad=pad_token_id)
        proc_bytes = ops.sample_proc_params(repetition_penalty, min_new_tokens)
        proc = float(repetition_penalty) != 1.0 or int(min_new_tokens) > 0
        greedy = not do_sample or float(temperature) <= 0
        logits, idle = self._first_logits(input_ids, attention_mask, extend)
        before = self._gen
        g = self._gen_state(logits.shape[-1], max_new_tokens, logprobs=logprobs)
        moved = before["history"] if before is not None and before is not g and before["vocab"] == g["vocab"] else None
        # Graphs and sampler kernels: without the processors the sampler is launched without proc / history (the kernels that
        # read neither) and captured into gen_graphs / row_gen_graphs; attaching them always would give the same tokens at
        # repetition_penalty = 1, slower.  greedy: one pass only, in graphs of its own key.  logprobs: the same sampler call with
        # the log-prob launch behind it, in lp_gen_graphs / row_lp_gen_graphs.
        def sample(lg):
            self._sample(lg, g, False, greedy, proc)
            if logprobs:
                self._logprob(lg, g)

        if logprobs:
            advance = (self.lp_gen_graphs, self.row_lp_gen_graphs, (greedy, proc))
        else:
            advance = (self.proc_gen_graphs, self.row_proc_gen_graphs, greedy) if proc else (self.gen_graphs, self.row_gen_graphs, greedy)
        return self._generate_loop(input_ids, logits, idle, extend, check_every, {
            "g": g, "words": {"params": params, "proc": proc_bytes} if proc else {"params": params}, "sample": sample,
            "advance": advance, "eos": [eos] * self.batch, "budgets": [max_new_tokens] * self.batch, "per_row": False, "proc": proc,
            "moved": moved, "logprobs": logprobs})

    @torch.inference_mode()
    def score(self, input_ids, attention_mask=None):
        """input_ids [batch, S] -> fp32 [batch, S] on the device: entry [b, s] is the log-probability of input_ids[b, s] given the
        row's real tokens before it, under the model's own distribution (ops.token_logprobs: no temperature, no warper, no logit
        processor).  The first real token of a row and every masked slot (attention_mask as in `prefill`) hold 0.0.  One
        `prefill` and one launch over its [batch, S, vocab] logits with the labels shifted by one -- no fp32 copy of the logits.
        The decoder is left exactly where `prefill` leaves it: `step` or `generate(..., extend=True)` can follow.  Perplexity of
        the batch, with n_scored the number of scored tokens (mask.sum() - batch; S - 1 per row without a mask):

            ppl = torch.exp(-dec.score(ids, mask).sum() / n_scored)"""
        input_ids = input_ids.to(self.device)
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch or input_ids.shape[1] < 1:
            raise ValueError(f"input_ids must be [{self.batch}, S >= 1], got {tuple(input_ids.shape)}")
        logits = self.prefill(input_ids, attention_mask)
        # slot s scores the token at s + 1; -1 (an ignored slot) in the last one and wherever either side is masked
        labels = torch.full(input_ids.shape, -1, dtype=torch.int64, device=self.device)
        labels[:, :-1] = input_ids[:, 1:]
        if attention_mask is not None:
            real = torch.as_tensor(attention_mask).to(self.device) != 0
            labels[:, :-1].masked_fill_(~(real[:, 1:] & real[:, :-1]), -1)
        lp = ops.token_logprobs(logits, labels)
        out = torch.zeros_like(lp)
        out[:, 1:] = lp[:, :-1]
        return out
