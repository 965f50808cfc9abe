#!/usr/bin/env python3
"""awq_prefill_attention_rows with equal rows against awq_prefill_attention on the same inputs: B 8 x S 2048 x 32 / 8 heads, start 0
and 2048, device events, the two forms alternating window by window.  The record is profiles/prefill_rows.txt:

    python tools/bench_prefill_rows.py > profiles/prefill_rows.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autoawq_amd import ops  # noqa: E402

B, S, Hq, Hkv, D = 8, 2048, 32, 8, 128
Tmax = 4096
gen = torch.Generator().manual_seed(0)
q = torch.randn((B, S, Hq, D), generator=gen).half().cuda()
k = torch.randn((B, Tmax, Hkv, D), generator=gen).half().cuda()
v = torch.randn((B, Tmax, Hkv, D), generator=gen).half().cuda()
out = torch.empty_like(q)
lines = [f"B {B} x S {S} x {Hq} / {Hkv} heads, head_dim {D}, cache window {Tmax}; device events, {12} windows of {20} launches each, "
         "the two forms alternating window by window; ms per launch"]


def window(fn, n=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


for start in (0, 2048):
    pos = torch.full((B,), start, dtype=torch.int32, device="cuda")
    cnt = torch.full((B,), S, dtype=torch.int32, device="cuda")
    shared = lambda: ops.prefill_attention(q, k, v, start)  # noqa: E731
    rows = lambda: ops.prefill_attention_rows(q, k, v, pos, cnt, start + S, out=out)  # noqa: E731
    same = torch.equal(shared().view(torch.int16), rows().view(torch.int16))
    for _ in range(3):
        window(shared), window(rows)
    ts, tr = [], []
    for _ in range(12):
        ts.append(window(shared))
        tr.append(window(rows))
    for name, t in (("awq_prefill_attention     ", ts), ("awq_prefill_attention_rows", tr)):
        lines.append(f"start {start:4d}  {name}  median {statistics.median(t):.4f}  min {min(t):.4f}  max {max(t):.4f}  "
                     f"spread (max - min) / median {(max(t) - min(t)) / statistics.median(t) * 100:.2f} %")
    d = statistics.median(tr) / statistics.median(ts) - 1
    lines.append(f"start {start:4d}  rows / shared - 1 = {d * 100:+.2f} %   outputs bit-identical: {same}")
print("\n".join(lines))
