#!/usr/bin/env python3
"""Time of the sampler's slots launch (awq_sample_tokens_slots) against the rows launch (awq_sample_tokens_rows) on as many rows,
and the replays speculative sampling needs on the tiny model, MI355X.

    python tools/bench_sample_slots.py [--out profiles/spec_sampling.txt] [--launches 50] [--rounds 9]

Launch time: V = 32000, B x T in {1 x 4, 1 x 8, 4 x 8} (4, 8 and 32 logits rows) x {greedy, sampled (temperature 0.7, top_k 50,
top_p 0.9)}, processors attached on both sides (penalty 1.1).  The rows form runs B * T independent rows on the same logits: the
same passes and combines; its kernels are, instruction for instruction, those of the commit before the slots form (DESIGN.md
3.10), so it is the baseline.  The slots form differs by the draft compare in process8 (<= 7 block-uniform ids), by reading cnt
and tok instead of t, and by writing no t / ring / history word.  Method as tools/bench_sample_rows.py: per case
one captured graph of `--launches` back-to-back launches per form, warmed up, then `--rounds` rounds that ALTERNATE the graphs,
each timed with device events over a window of >= 20 ms; the rows graph is measured twice per round (rows, rows2), so that the
spread of the baseline against itself is on the page.  Reported: median us per launch [min .. max], slots / rows.

Replays: generate(draft_tokens=3, draft_accept="sampler", do_sample=True) on the committed tiny-Llama checkpoint (gemm), three
prompts of 9 / 4 / 12 tokens, 40 new tokens (the 64-row cache window holds no more), temperature in {0.3, 0.7, 1.0}: the replays
the slowest row needed, and that figure scaled to 64 tokens.  No GPU: the script fails, it has no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autoawq_amd import ops  # noqa: E402

CASES = [(1, 4), (1, 8), (4, 8)]
V = 32000
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1)


def build(B, T, sampled, launches, stream):
    dev, R = "cuda", B * T
    g = torch.Generator().manual_seed(R * 7 + V)
    x = (torch.randn((R, V), generator=g) * 3).half().to(dev)
    cfg = SAMPLED if sampled else dict(do_sample=False)
    tok = torch.randint(0, V, (B, T), generator=g).to(dev)
    forms = {}
    for name in ("rows", "slots"):
        n = B if name == "slots" else R
        buf = {"out": torch.zeros(R, dtype=torch.int64, device=dev), "status": torch.zeros((R + 31) // 32, dtype=torch.int32, device=dev),
               "ws": torch.zeros(ops.sample_workspace_bytes(R, V), dtype=torch.uint8, device=dev),
               "params": ops.sample_params_rows(n, **cfg).to(dev), "proc": ops.sample_proc_params_rows(n, 1.1, 0).to(dev),
               "history": torch.zeros((n, ops.sample_history_words(V)), dtype=torch.int32, device=dev),
               "t": torch.ones(n, dtype=torch.int32, device=dev)}
        if name == "slots":
            def run(buf=buf):
                ops.sample_launch_slots(x, buf["params"], buf["t"], tok, buf["out"], buf["status"], buf["ws"], greedy=not sampled,
                                        proc=buf["proc"], history=buf["history"])
        else:
            def run(buf=buf):
                ops.sample_launch_rows(x, buf["params"], buf["t"], buf["out"], buf["status"], buf["ws"], greedy=not sampled,
                                       proc=buf["proc"], history=buf["history"])
        run()
        torch.cuda.synchronize()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(launches):
                    run()
        buf["graph"] = graph
        forms[name] = buf
    return forms


def time_graph(graph, replays, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        for _ in range(replays):
            graph.replay()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / replays   # us per replay


def replays_on_the_tiny_model(lines):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_spec_generate import _decoder, _left_padded, _prompts

    ids, mask = _left_padded(_prompts([9, 4, 12]))
    n = 40
    lines.append(f"# replays: tiny-Llama (gemm), prompts of 9 / 4 / 12 tokens, {n} new tokens, draft_tokens = 3, seed 1")
    for temperature in (0.3, 0.7, 1.0):
        dec = _decoder("gemm", 3)
        dec.generate(ids, max_new_tokens=n, draft_tokens=3, draft_accept="sampler", do_sample=True, temperature=temperature, seed=1,
                     attention_mask=mask)
        r = dec.last_spec["replays"]
        lines.append(f"temperature {temperature}: {r} replays for {n} tokens = {r * 64 / n:.1f} per 64 tokens (plain: {n - 1} / {63})")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_slots: needs an MI355X (no fallback)")
    stream = torch.cuda.Stream()
    lines = [f"# tools/bench_sample_slots.py: us per launch inside a graph of {a.launches} launches, median [min .. max] of {a.rounds} "
             "alternating rounds", f"# device: {torch.cuda.get_device_name(0)}",
             f"# B x T, mode (V = {V}): rows | rows again | slots | slots / rows"]
    for B, T in CASES:
        for sampled in (False, True):
            forms = build(B, T, sampled, a.launches, stream)
            for f in forms.values():                       # warm-up, and the replay count for a >= 20 ms window
                time_graph(f["graph"], 3, stream)
            per = time_graph(forms["rows"]["graph"], 5, stream)
            replays = max(5, int(20000.0 / max(per, 1.0)) + 1)
            got = {"rows": [], "rows2": [], "slots": []}
            for r in range(a.rounds):
                for name in (("rows", "slots", "rows2") if r % 2 == 0 else ("slots", "rows2", "rows")):
                    got[name].append(time_graph(forms["rows" if name == "rows2" else name]["graph"], replays, stream) / a.launches)
            med = {k: statistics.median(v) for k, v in got.items()}
            rec = {"B": B, "T": T, "V": V, "mode": "sampled" if sampled else "greedy", "launches": a.launches, "replays": replays,
                   **{k + "_us": v for k, v in med.items()}, "ratio": med["slots"] / med["rows"],
                   **{k + "_min_max": [min(v), max(v)] for k, v in got.items()}}
            print(json.dumps(rec), flush=True)
            cell = {k: f"{med[k]:7.2f} [{min(v):.2f} .. {max(v):.2f}]" for k, v in got.items()}
            lines.append(f"{B} x {T} {rec['mode']:8s}: {cell['rows']} | {cell['rows2']} | {cell['slots']} | {rec['ratio']:.3f}")
    replays_on_the_tiny_model(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
