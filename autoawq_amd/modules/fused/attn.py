"""QuantAttentionFused for MI355X (reference: awq/modules/fused/attn.py:127-312).

Same constructor arguments and the same forward contract: `forward(hidden_states)` runs the fused qkv projection, rotary
embedding, the KV-cache update, attention and `o_proj`, advances `start_pos`, and returns `(attn_output, attention_weight,
past_key_value)`.  Everything after the projection is `forward_qkv`: it states what the call is as ONE `AttnStep` (`_step`), and
the append, the rows attended over and the attention kernel are read off that description and nothing else:

  kind     asked for by           positions from                     append (rope_kv_append)   attention                   start_pos
  prefill  S > 1                  host start_pos                     S rows at start_pos       prefill_attention [1]       += S
  decode   S == 1                 host start_pos, or                 one row at the position   decode_attention; append    += 1
                                  shared words (pos, len), or                                  and attention in ONE launch
                                  per-row words [B]                                            (decode_attention_rope) [2]
  verify   request="verify"       per-row words                      T rows at pos_b           verify_attention_rows       stays
  extend   request=(pos, count,   per-row pos and count, host bound  count_b rows at pos_b     prefill_attention_rows      stays
           max_end)               max_end                                                      (max_end == 0: zeros)

  [1] head_dim 128 and PREFILL_KERNEL; otherwise the vendor's attention (`_attend_vendor`: fp32 matmul-softmax when the scores
      carry a soft cap or ALiBi, else scaled_dot_product_attention), which decode takes too on a non-native head shape.
  [2] one launch for rotation, append and attention: native head shape, full rotary, FUSE_ROPE_INTO_ATTENTION, no modifier.

  * native head shape: head_dim 128 and 1, 2, 4 or 8 query heads per KV head (what the hand-written decode, verify and rows
    kernels take).  Per-row words, verify, extend and the fp8 cache need it.
  * `use_device_positions(pos, len, per_row, bound)`: decode positions live in device int32 words so that one captured hipGraph
    serves every step; a launch whose length only the device knows is sized for `bound` (default: the cache window).  verify and
    extend are never inferred from S: the caller asks for them, owns the positions and keeps only the rows it wants.
  * `attention_shapes` and `q_norm` / `k_norm` (attn.py:89-125,159-203) are applied to the projection's output, which is put back
    into the q | k | v head order the kernels read (`_qkv_rows`); ALiBi models skip the rotation (rotary width 0 in the append) and
    pass their slopes, `attn_logit_softcapping` its cap, to the kernels (the reference: `alibi_slopes=` / `softcap=`, :286-302).
  * `kv_cache_dtype="fp8"` (opt-in): the cache holds e4m3 codes + one fp32 scale per row (WindowedCache, format in
    include/awq_hip.h); append and decode run the *_fp8 kernels.  prefill and extend append codes, dequantize rows [0, end) into an
    fp16 workspace (`_kv_rows`) and attend over that, so a prompt sees the values its decode steps will read."""
import math
import os
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from .cache import WindowedCache


class RoPE(nn.Module):
    """cos / sin tables [max_seq_len, rotary_dim / 2] fp32: the real and imaginary parts of
    `precompute_freqs_cis` (attn.py:37-43)."""

    def __init__(self, head_dim, max_seq_len, device, rope_theta):
        super().__init__()
        self.head_dim = head_dim
        freqs = 1.0 / (rope_theta ** (torch.arange(0, head_dim, 2)[: (head_dim // 2)].float() / head_dim))
        t = torch.arange(max_seq_len)
        freqs = torch.outer(t, freqs).float()
        self.register_buffer("cos", freqs.cos().contiguous().to(device), persistent=False)
        self.register_buffer("sin", freqs.sin().contiguous().to(device), persistent=False)


class ALiBi(nn.Module):
    """Slopes [n_heads] and the bias row of the last query [1, n_heads, 1, max_seq_len] (attn.py:89-125): head h adds
    slope_h * (key position - query position) to its scores.  `forward(scores, seqlen)` like the reference's."""

    def __init__(self, n_heads, max_seq_len, device, alibi_bias_max=8):
        super().__init__()
        slopes, bias = self.build_alibi_bias(n_heads, max_seq_len, alibi_bias_max=alibi_bias_max)
        self.slopes = nn.Parameter(slopes.float().to(device), requires_grad=False)
        self.bias = nn.Parameter(bias.float().to(device), requires_grad=False)

    @staticmethod
    def gen_slopes(n_heads, alibi_bias_max=8):
        pow2 = 1 << max(0, math.ceil(math.log2(n_heads)))
        exponents = torch.arange(1, pow2 + 1, dtype=torch.float32) * (alibi_bias_max / pow2)
        slopes = torch.pow(2.0, exponents).reciprocal()
        if pow2 != n_heads:  # the odd exponents first, then the even ones, cut to n_heads
            slopes = torch.cat([slopes[1::2], slopes[0::2]])[:n_heads]
        return slopes.view(1, n_heads, 1, 1)

    @staticmethod
    def build_alibi_bias(n_heads, seq_len, alibi_bias_max=8, dtype=torch.float32):
        slopes = ALiBi.gen_slopes(n_heads, alibi_bias_max)
        distance = torch.arange(1 - seq_len, 1, dtype=torch.int32).view(1, 1, 1, seq_len)
        return slopes.reshape(n_heads).to(dtype), (distance * slopes).to(dtype)

    def forward(self, scores, seqlen):
        scores += self.bias[..., :seqlen]
        return scores


class AttnStep(NamedTuple):
    """What one forward_qkv call is (QuantAttentionFused._step builds it; the table in the module docstring reads it)."""
    kind: str             # "prefill" | "decode" | "verify" | "extend"
    seqlen: int
    start: int            # the host's start_pos; 0 where the caller owns the positions (verify, extend)
    pos: object = None    # device position word(s) -- None: the positions are `start`, on the host
    len: object = None    # device length word(s) after the append (decode)
    rows: bool = False    # pos / len (/ count) hold one word per sequence, not one shared word
    count: object = None  # extend: new tokens per sequence
    bound: object = None  # what a launch with a device-side length is sized for (extend: max_end); None on the host

    @property
    def advance(self):
        """the module's start_pos moves by seqlen (verify and extend: the caller owns the positions)"""
        return self.kind in ("prefill", "decode")

    @property
    def end(self):
        """host bound of the cache rows this call may see"""
        return self.bound if self.kind == "extend" else self.start + self.seqlen

    def word(self, w):
        """(shared word, per-row words): the two keyword slots the kernels have for one device word"""
        return (None, w) if self.rows else (w, None)


class QuantAttentionFused(nn.Module):
    FUSE_ROPE_INTO_ATTENTION = True  # decode steps, head_dim 128, full rotary
    PREFILL_KERNEL = True            # prefill steps, head_dim 128: csrc/prefill_attn.hip (False: the vendor's attention, for A/B runs)

    def __init__(self, hidden_size, n_heads, n_kv_heads, qkv_layer, o_proj, dev, max_seq_len=2048, use_alibi=False,
                 attention_shapes=None, rope_theta=10000, partial_rotary_factor=1.0, head_dim=None,
                 attn_logit_softcapping=0.0, q_norm=None, k_norm=None, kv_cache_dtype="fp16", **kwargs):
        super().__init__()
        from ...utils.fused_utils import get_attention_shapes

        self.hidden_size = hidden_size
        self.n_heads = n_heads
        self.n_kv_heads = n_kv_heads if n_kv_heads != 0 else n_heads
        self.n_kv_groups = n_heads // self.n_kv_heads
        self.head_dim = head_dim if head_dim is not None else hidden_size // n_heads
        self.qkv_proj = qkv_layer
        self.o_proj = o_proj
        self.start_pos = 0
        self.use_alibi = bool(use_alibi)
        self.q_norm, self.k_norm = q_norm, k_norm
        self.attn_logit_softcapping = float(attn_logit_softcapping or 0.0)
        self._custom_shapes = attention_shapes is not None
        self.attention_shapes = get_attention_shapes(attention_shapes, n_heads, n_kv_heads, self.head_dim)
        if kv_cache_dtype not in ("fp16", "fp8"):
            raise ValueError(f"QuantAttentionFused: kv_cache_dtype must be 'fp16' or 'fp8', got {kv_cache_dtype!r}")
        if kv_cache_dtype == "fp8" and not (self.native and n_heads % self.n_kv_heads == 0):
            raise ValueError(f"QuantAttentionFused: kv_cache_dtype='fp8' needs head_dim 128 and 1, 2, 4 or 8 query heads per KV head "
                             f"(got head_dim {self.head_dim}, {n_heads} / {self.n_kv_heads} heads)")
        self.kv_cache_dtype = kv_cache_dtype
        self.cache_batch_size = int(os.getenv("AWQ_BATCH_SIZE", "1"))
        if kwargs.get("max_length") is not None:
            max_seq_len = kwargs["max_length"]
        self.max_seq_len = max_seq_len
        self.is_hf_transformers = False
        self.rope_theta = rope_theta
        self.cache = WindowedCache(self.cache_batch_size, n_heads, self.n_kv_heads, self.head_dim, max_seq_len, dev,
                                   dtype=kv_cache_dtype)
        self.partial_rotary_factor = partial_rotary_factor
        if self.use_alibi:  # no rotation (attn.py:189-194,254): the append kernel runs with rotary width 0
            self.alibi = ALiBi(n_heads, max_seq_len, dev)
            self.rotary_dim = 0
            self.rope = RoPE(2, 1, dev, rope_theta)  # (tables the kernel never reads)
            self.is_neox = False
        else:
            self.alibi = None
            self.rotary_dim = int(self.head_dim * partial_rotary_factor)
            self.rope = RoPE(self.rotary_dim, max_seq_len, dev, rope_theta)
            self.is_neox = True
        self._pos_dev = self._len_dev = self._bound = None
        self._per_row = False

    @property
    def native(self):
        """the head shapes the hand-written decode, verify and rows kernels take; others run the vendor's attention"""
        return self.head_dim == 128 and self.n_kv_groups in (1, 2, 4, 8)

    @property
    def modified(self):
        """the scores carry a bias (ALiBi) or a cap: no fused decode launch, fp32 scores on the vendor path"""
        return self.alibi is not None or self.attn_logit_softcapping > 0

    def use_device_positions(self, pos_dev, len_dev, per_row=False, bound=None):
        """pos_dev / len_dev: int32 device tensors of one element (shared by all layers) holding the
        start position and the cache length after the append; the caller advances them.  per_row=True: both are [B], one
        position and one length per sequence (decode steps only; the host-side start_pos of prefill is not per row).
        bound: what a launch that reads its length from the device is sized for -- the cache window, or the tighter bound of a
        caller that knows the context on the host (modules/fused/decode.py: one hipGraph per length bucket).  (None, None): back
        to the host's start_pos, and the bound goes with the words."""
        if per_row and (pos_dev is None or len_dev is None):
            raise ValueError("use_device_positions: per_row needs both the position and the length words")
        self._pos_dev, self._len_dev, self._per_row = pos_dev, len_dev, bool(per_row)
        self._bound = None if pos_dev is None else self.max_seq_len if bound is None else max(1, min(int(bound), self.max_seq_len))

    def _resize_cache(self, bsz):
        if bsz != self.cache_batch_size:
            if bsz > self.cache_batch_size:
                self.cache.increase_batch_size(bsz)
            else:
                self.cache.decrease_batch_size(bsz)
            self.cache_batch_size = bsz
            self.start_pos = 0  # the reference resets on a batch-size change (attn.py:208-218)

    def forward(self, hidden_states, *args, request=None, **kwargs):
        bsz, seqlen, _ = hidden_states.shape
        self._resize_cache(bsz)
        xqkv = self.qkv_proj(hidden_states)
        if xqkv.dtype != torch.float16:
            xqkv = xqkv.half()
        return self.forward_qkv(xqkv, request=request)

    def _qkv_rows(self, xqkv):
        """The projection's output as the kernels read it: [B, S, (Hq + 2 Hkv) * D], q heads | k heads | v heads.  Custom
        `attention_shapes` and q / k norms are applied on the reference's views (attn.py:244-253) and the three tensors joined
        again; without them (the default view IS that order) the tensor passes through untouched."""
        if not self._custom_shapes and self.q_norm is None and self.k_norm is None:
            return xqkv
        B, S, _ = xqkv.shape
        sh = self.attention_shapes
        v = xqkv.view((B, S) + tuple(sh["xqkv_view"]))
        xq, xk, xv = sh["xq_slice"](v), sh["xk_slice"](v), sh["xv_slice"](v)
        xq = xq.reshape(B, S, self.n_heads, self.head_dim)
        xk = xk.reshape(B, S, self.n_kv_heads, self.head_dim)
        xv = xv.reshape(B, S, self.n_kv_heads, self.head_dim)
        if self.q_norm is not None:
            xq = self.q_norm(xq)
        if self.k_norm is not None:
            xk = self.k_norm(xk)
        return torch.cat([xq.reshape(B, S, -1), xk.reshape(B, S, -1), xv.reshape(B, S, -1)], dim=-1).to(torch.float16).contiguous()

    def _attend_torch(self, q, k, v, first_q_pos):
        """q [B, Hq, S, D], k / v [B, Hq, T, D]: causal attention with the score modifiers, fp32 (prefill with soft-capping
        or ALiBi; decode for head shapes the hand-written kernel does not take)."""
        scores = torch.matmul(q.float(), k.float().transpose(-1, -2)) * (self.head_dim ** -0.5)
        if self.attn_logit_softcapping:
            scores = self.attn_logit_softcapping * torch.tanh(scores / self.attn_logit_softcapping)
        qpos = first_q_pos + torch.arange(q.shape[2], device=q.device).view(-1, 1)
        kpos = torch.arange(k.shape[2], device=q.device).view(1, -1)
        if self.alibi is not None:
            scores = scores + self.alibi.slopes.view(1, -1, 1, 1) * (kpos - qpos).float()
        scores = scores.masked_fill(kpos > qpos, float("-inf"))
        return torch.matmul(torch.softmax(scores, dim=-1), v.float()).to(torch.float16)

    def _step(self, seqlen, request):
        """The one place that reads the configured words and the call: request None (prefill for S > 1, else decode), "verify"
        (T = 2 .. 8 tokens per sequence at the per-row words: speculative decoding) or (pos_rows, count_rows, max_end) (extend:
        sequence b's first count_rows[b] tokens at cache rows pos_rows[b] .., max_end the host's bound of their sums)."""
        if request == "verify":
            if self.kv_cache_dtype == "fp8":
                raise NotImplementedError('speculative decoding: kv_cache_dtype="fp8" is not supported (verify_attention_rows '
                                          "reads fp16 caches)")
            if not (self._per_row and self._pos_dev is not None):
                raise RuntimeError("a verify step needs per-row device positions (use_device_positions(..., per_row=True))")
            if not self.native or self.modified or not 2 <= seqlen <= 8:
                raise NotImplementedError("a verify step takes 2 .. 8 tokens, head_dim 128, 1, 2, 4 or 8 query heads per KV head, "
                                          "no ALiBi and no soft cap")
            return AttnStep("verify", seqlen, 0, self._pos_dev, rows=True, bound=max(seqlen, self._bound))
        if request is not None:
            pos_rows, count_rows, max_end = request
            max_end = int(max_end)
            if not self.native:
                raise NotImplementedError("an extend step takes head_dim 128 and 1, 2, 4 or 8 query heads per KV head")
            if not 0 <= max_end <= self.max_seq_len:
                raise ValueError(f"extend: max_end {max_end} outside the cache window {self.max_seq_len}")
            return AttnStep("extend", seqlen, 0, pos_rows, rows=True, count=count_rows, bound=max_end)
        if seqlen > 1 or self._pos_dev is None:  # (prefill is at the host's start_pos whether words are set or not)
            return AttnStep("prefill" if seqlen > 1 else "decode", seqlen, self.start_pos)
        return AttnStep("decode", seqlen, self.start_pos, self._pos_dev, self._len_dev, self._per_row, bound=self._bound)

    def _kv_rows(self, step, bsz):
        """what a prefill-type kernel attends over: the caches themselves, or rows [0, end) of an fp8 cache dequantized to fp16
        [B, end, Hkv, 128]"""
        c = self.cache
        if self.kv_cache_dtype != "fp8" or step.kind == "decode":
            return c.k, c.v
        return ops.kv_dequant_fp8(c.k, c.k_scale, step.end, bsz), ops.kv_dequant_fp8(c.v, c.v_scale, step.end, bsz)

    def _attend_vendor(self, step, xq, k_rows, v_rows, bsz):
        """head shapes the hand-written kernels do not take (e.g. 24 / 8 heads, head_dim 64), or PREFILL_KERNEL off: the vendor's
        attention over rows [0, end) -> [B, S, Hq, D]"""
        q = xq.transpose(1, 2)                                      # [B, Hq, S, D]
        k = k_rows[:bsz, :step.end].transpose(1, 2)                 # [B, Hkv, T, D]
        v = v_rows[:bsz, :step.end].transpose(1, 2)
        if self.n_kv_groups > 1:
            k = k.repeat_interleave(self.n_kv_groups, dim=1)
            v = v.repeat_interleave(self.n_kv_groups, dim=1)
        if self.modified:  # fp32 matmul softmax when the scores carry a bias or a cap
            out = self._attend_torch(q, k, v, step.start)
        elif step.kind == "decode":
            out = F.scaled_dot_product_attention(q, k, v)
        elif step.start == 0:
            out = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        else:  # chunked prefill: query s sees cache rows <= start_pos + s
            mask = torch.ones((step.seqlen, step.end), dtype=torch.bool, device=q.device).tril(diagonal=step.start)
            out = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        return out.transpose(1, 2)

    def _attend(self, step, xq, bsz):
        """xq [B, S, Hq, D], rotated, its k / v rows already in the cache -> the heads' output"""
        c, softcap = self.cache, self.attn_logit_softcapping
        slopes = self.alibi.slopes if self.alibi is not None else None
        if step.kind == "verify":  # query (b, j) attends over rows <= pos_b + j
            return ops.verify_attention_rows(xq, c.k, c.v, step.pos, max_len=step.bound)
        if step.kind == "extend" and step.end == 0:  # no row has a token and none a context: nothing to attend
            return torch.zeros_like(xq)
        k_rows, v_rows = self._kv_rows(step, bsz)
        if step.kind == "extend":  # query (b, s) attends over rows <= pos_b + s; the slots behind count_b are zeros
            return ops.prefill_attention_rows(xq, k_rows, v_rows, step.pos, step.count, step.end, softcap=softcap, alibi_slopes=slopes)
        if step.kind == "prefill" and self.head_dim == 128 and self.n_heads % self.n_kv_heads == 0 and self.PREFILL_KERNEL:
            # the hand-written flash-style kernel (csrc/prefill_attn.hip; the reference's flash_attn_func call, attn.py:269-277),
            # chunked prefill, GQA, ALiBi and the soft cap included -- no mask tensor, no repeat_interleave copy of the cache
            return ops.prefill_attention(xq, k_rows, v_rows, step.start, softcap=softcap, alibi_slopes=slopes)
        if step.kind == "decode" and self.native:
            len_dev, len_rows = step.word(step.len)
            # max_len only with a device length (step.bound is None on the host): the launcher sizes the split from seq_len then
            # and never reads it (csrc/decoder.hip, awq_launch_decode_attention)
            return ops.decode_attention(xq[:, 0], c.k, c.v, step.start + 1, len_dev=len_dev, max_len=step.bound, softcap=softcap,
                                        alibi_slopes=slopes, len_rows=len_rows, k_scale=c.k_scale, v_scale=c.v_scale)
        if step.rows:
            raise NotImplementedError("per-row decode positions need the native decode attention (head_dim 128, "
                                      "1, 2, 4 or 8 query heads per KV head)")
        return self._attend_vendor(step, xq, k_rows, v_rows, bsz)

    def forward_qkv(self, xqkv, apply_o_proj=True, request=None):
        """Everything after the qkv projection (the caller may have produced `xqkv` [B, S, (Hq + 2 Hkv) D]
        with the norm folded into the projection).  apply_o_proj=False returns the attention heads' output
        in place of attn_output (the caller runs o_proj with the residual add in its epilogue).  request: see `_step`."""
        bsz, seqlen, _ = xqkv.shape
        self._resize_cache(bsz)
        xqkv = self._qkv_rows(xqkv)
        step = self._step(seqlen, request)
        c, rope = self.cache, self.rope
        pos_dev, pos_rows = step.word(step.pos)
        if (step.kind == "decode" and self.native and self.rotary_dim == 128 and self.FUSE_ROPE_INTO_ATTENTION
                and not self.modified):
            # rotation, cache append and attention in ONE launch (awq_decode_attention_rope); max_len as in `_attend`
            out = ops.decode_attention_rope(xqkv, c.k, c.v, rope.cos, rope.sin, step.start, self.n_heads, self.n_kv_heads,
                                            pos_dev=pos_dev, max_len=step.bound, pos_rows=pos_rows, k_scale=c.k_scale,
                                            v_scale=c.v_scale)
        else:
            xq = ops.rope_kv_append(xqkv, c.k, c.v, rope.cos, rope.sin, step.start, self.n_heads, self.n_kv_heads, self.head_dim,
                                    self.rotary_dim, pos_dev=pos_dev, pos_rows=pos_rows, k_scale=c.k_scale, v_scale=c.v_scale,
                                    count_rows=step.count)
            out = self._attend(step, xq, bsz)
        attention_weight = out.reshape(bsz, seqlen, -1)
        attn_output = self.o_proj(attention_weight) if apply_o_proj else attention_weight
        if step.advance:
            self.start_pos += seqlen
        return attn_output, attention_weight, [torch.zeros(1, 1, self.start_pos, 1)]
