#!/usr/bin/env python3
"""Time of the sampler's rows launch (awq_sample_tokens_rows) against the shared launch (awq_sample_tokens), MI355X.

    python tools/bench_sample_rows.py [--out profiles/sample_rows.txt] [--launches 50] [--rounds 9]

B in {1, 8, 64} x V in {32000, 128256} x {greedy, sampled (temperature 0.7, top_k 50, top_p 0.9)}.  Both forms get the same
logits, the same parameters in every row and the same token index, so they do the same work and emit the same tokens (checked
before timing); the rows form differs by one indexed 64-byte parameter read and one 4-byte t[r] read per block, and by each row
advancing its own t.  The shared launch's kernels are, instruction for instruction, those of the commit before the rows form
(DESIGN.md 3.10), so it is the baseline.

Method: per case one captured graph of `--launches` back-to-back launches per form (no host launch cost in the window), warmed
up, then `--rounds` rounds that ALTERNATE the two graphs, each replay timed with device events around enough replays for a window
of >= 20 ms.  Reported: the median us per launch of each form, the min .. max over the rounds (the run-to-run spread the
difference has to be read against), and the ratio of the medians.  No GPU: the script fails, it has no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autoawq_amd import ops  # noqa: E402

CASES = [(B, V) for V in (32000, 128256) for B in (1, 8, 64)]
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1)


def build(B, V, sampled, launches, stream):
    dev = "cuda"
    g = torch.Generator().manual_seed(B * 7 + V)
    x = (torch.randn((B, V), generator=g) * 3).half().to(dev)
    cfg = SAMPLED if sampled else dict(do_sample=False)
    forms = {}
    for name in ("shared", "rows"):
        rows = name == "rows"
        buf = {"t": torch.ones(B if rows else 1, dtype=torch.int32, device=dev),
               "out": torch.zeros(B, dtype=torch.int64, device=dev),
               "status": torch.zeros((B + 31) // 32, dtype=torch.int32, device=dev),
               "ws": torch.zeros(ops.sample_workspace_bytes(B, V), dtype=torch.uint8, device=dev),
               "params": (ops.sample_params_rows(B, **cfg) if rows else ops.sample_params(**cfg)).to(dev)}
        launch = ops.sample_launch_rows if rows else ops.sample_launch

        def run(buf=buf, launch=launch):
            launch(x, buf["params"], buf["t"], buf["out"], buf["status"], buf["ws"], greedy=not sampled)

        run()
        torch.cuda.synchronize()
        buf["first"] = buf["out"].clone()
        buf["t"].fill_(1)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(launches):
                    run()
        buf["graph"] = graph
        forms[name] = buf
    if not torch.equal(forms["shared"]["first"], forms["rows"]["first"]):
        raise RuntimeError(f"B = {B}, V = {V}: the two forms emit different tokens")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_rows: needs an MI355X (no fallback)")
    stream = torch.cuda.Stream()
    lines = [f"# tools/bench_sample_rows.py: us per launch inside a graph of {a.launches} launches, median [min .. max] of {a.rounds} "
             "alternating rounds", f"# device: {torch.cuda.get_device_name(0)}",
             "# B, V, mode: shared | rows | rows / shared"]
    for B, V in CASES:
        for sampled in (False, True):
            forms = build(B, V, sampled, a.launches, stream)
            for f in forms.values():                       # warm-up, and the replay count for a >= 20 ms window
                time_graph(f["graph"], 3, stream)
            per = time_graph(forms["shared"]["graph"], 5, stream)
            replays = max(5, int(20000.0 / max(per, 1.0)) + 1)
            got = {"shared": [], "rows": []}
            for r in range(a.rounds):
                for name in (("shared", "rows") if r % 2 == 0 else ("rows", "shared")):
                    got[name].append(time_graph(forms[name]["graph"], replays, stream) / a.launches)
            med = {k: statistics.median(v) for k, v in got.items()}
            rec = {"B": B, "V": V, "mode": "sampled" if sampled else "greedy", "launches": a.launches, "replays": replays,
                   "shared_us": med["shared"], "rows_us": med["rows"], "ratio": med["rows"] / med["shared"],
                   "shared_min_max": [min(got["shared"]), max(got["shared"])], "rows_min_max": [min(got["rows"]), max(got["rows"])]}
            print(json.dumps(rec), flush=True)
            lines.append(f"{B:3d} {V:7d} {rec['mode']:8s}: {med['shared']:7.2f} [{min(got['shared']):.2f} .. {max(got['shared']):.2f}] | "
                         f"{med['rows']:7.2f} [{min(got['rows']):.2f} .. {max(got['rows']):.2f}] | {rec['ratio']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
