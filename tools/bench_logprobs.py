#!/usr/bin/env python3
"""Token log-probabilities (csrc/logprob.hip), timed with device events.

1. The kernel alone -- ops.token_logprobs_launch captured `per` times into a graph and replayed -- beside what a user writes
   without it, torch.log_softmax(logits.float(), -1).gather(-1, ids), captured the same way on the same tensors.  Decode-sized
   row counts at two vocabularies and one scoring-sized batch; bytes = R V 2 (the logits, read once).
2. The whole decoder: GraphedDecoder.generate per token with and without logprobs=True on the synthetic Llama-2-7B-shape model
   of tools/bench_decode_model.py (GEMV layout, vocab 32000), context 64, batch 1, the two alternating so that they share
   whatever else the machine is doing.  The off path is the code a call without logprobs always ran.
--kernel-only / --decoder-only run one half."""
import argparse, json, os, statistics, sys, time
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ((1, 32000), (4, 32000), (64, 32000), (1, 128256), (4, 128256), (64, 128256), (4096, 32000))


def _graph_us(fn, per, replays):
    """fn captured `per` times into one graph; device-event time per call over `replays` replays (after one warm replay)"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(per):
                fn()
        g.replay()
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(replays):
            g.replay()
        e1.record(s)
        e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / (per * replays)


def bench_kernel(shapes=SHAPES):
    from autoawq_amd import ops

    dev = torch.device("cuda")
    rows = []
    for R, V in shapes:
        gen = torch.Generator(device=dev).manual_seed(R + V)
        x = (torch.randn((R, V), device=dev, generator=gen) * 3).half()
        ids = torch.randint(0, V, (R,), device=dev, generator=gen)
        out = torch.empty(R, dtype=torch.float32, device=dev)
        per, replays = (10, 50) if R * V < (1 << 24) else (2, 10)
        ours = _graph_us(lambda: ops.token_logprobs_launch(x, ids, out), per, replays)
        keep = []
        torch_us = _graph_us(lambda: keep.append(torch.log_softmax(x.float(), -1).gather(-1, ids.view(-1, 1))), per, replays)
        err = float((out.double() - torch.log_softmax(x.double(), -1).gather(-1, ids.view(-1, 1)).view(-1)).abs().max())
        r = {"R": R, "V": V, "kernel_us": round(ours, 2), "torch_log_softmax_gather_us": round(torch_us, 2),
             "kernel_GBps": round(R * V * 2 / ours / 1e3, 1), "speedup": round(torch_us / ours, 2), "max_abs_diff_vs_fp64": err}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del keep
    return rows


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_decoder(layers=32, ctx=64, B=1, new=128, rounds=7):
    import bench_decode_model
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    dev = torch.device("cuda")
    lm, blocks, gen = bench_decode_model.build_model(layers, ctx + new + 8, dev, layout="gemv")
    V = bench_decode_model.V
    dec = GraphedDecoder(lm, batch=B)
    prompt = torch.randint(0, V, (B, ctx), device=dev, generator=gen)
    dec.prefill(prompt)
    t_pre = min(_timed(lambda: dec.prefill(prompt)) for _ in range(3))
    legs = {"off": lambda: dec.generate(prompt, new), "on": lambda: dec.generate(prompt, new, logprobs=True)}
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()  # captures
    for _ in range(rounds):  # alternating
        for k, fn in legs.items():
            times[k].append(_timed(fn))
    assert dec.last_logprobs is not None and bool((dec.last_logprobs < 0).all())
    rows = []
    for k, ts in times.items():
        per_tok = [(t - t_pre) / (new - 1) * 1e6 for t in ts]
        r = {"batch": B, "context": ctx, "new_tokens": new, "logprobs": k, "prefill_s": round(t_pre, 5),
             "us_per_token_min": round(min(per_tok), 2), "us_per_token_median": round(statistics.median(per_tok), 2),
             "us_per_token_max": round(max(per_tok), 2), "decode_tok_s_best": round(B * 1e6 / min(per_tok), 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    d = {"logprobs_cost_us_per_token_min": round(rows[1]["us_per_token_min"] - rows[0]["us_per_token_min"], 2),
         "logprobs_cost_us_per_token_median": round(rows[1]["us_per_token_median"] - rows[0]["us_per_token_median"], 2)}
    print(json.dumps(d), flush=True)
    return rows + [d]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--decoder-only", action="store_true")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=128)
    a = ap.parse_args()
    if not a.decoder_only:
        bench_kernel()
    if not a.kernel_only:
        bench_decoder(layers=a.layers, new=a.new)
