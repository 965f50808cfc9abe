"""numpy restatement of the logit processors of csrc/sample.hip (awq_sample_tokens_ex, see its header comment): the `process`
step that precedes the contract of tests/sampling_ref.py, so the restatement of a processed launch is
sampling_ref.choose(process(...)).  The history is a per-row bitmap: bit v % 32 of int32 word v / 32 = token v seen."""
import numpy as np

FP16_MAX = np.float32(65504.0)


def words(V):
    return (int(V) + 31) // 32


def bitmap(rows, V, width=None):
    """rows: a list of id sequences (one per row) -> int32 [len(rows), width or ceil(V / 32)]; ids outside [0, V) ignored"""
    w = np.zeros((len(rows), width or words(V)), dtype=np.uint32)
    for r, ids in enumerate(rows):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        ids = ids[(ids >= 0) & (ids < V)]
        np.bitwise_or.at(w[r], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return w.view(np.int32)


def seen_mask(history_row, V):
    """bool [V] of one history row (int32 / uint32 words)"""
    w = np.asarray(history_row).view(np.uint32)
    i = np.arange(V)
    return ((w[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def process(logits, seen, *, t=1, repetition_penalty=1.0, min_new_tokens=0, eos_ids=()):
    """fp16 logits [V] -> the fp16 values every pass of the kernel reads.  seen: bool [V] (the row's history bits).
      1. t <= min_new_tokens: the EOS ids are -inf;
      2. otherwise a seen, finite logit: v < 0 ? v * p : v / p in fp32, rounded to fp16 (nearest even) saturating at +-65504;
         -inf / +inf / NaN unchanged."""
    h = np.asarray(logits, dtype=np.float16).copy()
    V = h.shape[0]
    seen = np.asarray(seen, dtype=bool)
    eos = np.zeros(V, dtype=bool)
    if t <= min_new_tokens:
        for e in eos_ids:
            if 0 <= int(e) < V:
                eos[int(e)] = True
    p = np.float32(repetition_penalty)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = h.astype(np.float32)
        pen = np.where(v < 0, v * p, v / p).astype(np.float32)
        pen = np.clip(pen, -FP16_MAX, FP16_MAX).astype(np.float16)
    apply = seen & np.isfinite(h) & ~eos
    out = np.where(apply, pen, h)
    out[eos] = np.float16(-np.inf)
    return out
