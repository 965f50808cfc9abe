#!/usr/bin/env python3
"""What a speculative verify step costs: on the synthetic 7B shape (tools/bench_decode_model.py, GEMV layout), one plain decode
replay against one verify replay at T = 2, 4, 8, at 64 and 2048 tokens of context, batch 1 and 4, in the same process.

ratio = verify / plain is the mean number of tokens a verify step has to emit for speculation to break even (a plain step
emits one); with acceptance of a draft independent with probability p a step emits (1 - p^T) / (1 - p) tokens.  The argmax,
acceptance and draft kernels of a full speculative replay are timed once beside it (spec - verify).

    python tools/spec_decode_probe.py > profiles/spec_decode.txt

Each figure: median of REPEATS timed runs of STEPS replays between two events on the decoder's stream, after WARM replays."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, REPEATS, WARM = 32, 5, 4


def timed(stream, fn, reset=None):
    out = []
    with torch.cuda.stream(stream):
        for _ in range(WARM):
            fn()
        for _ in range(REPEATS):
            if reset is not None:
                reset()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(STEPS):
                fn()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / STEPS)
    return statistics.median(out), min(out), max(out)


def main():
    import bench_decode_model as bdm
    from autoawq_amd import ops
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    a = ap.parse_args()
    dev = torch.device("cuda")
    contexts, Ts = (64, 2048), (2, 4, 8)
    print(f"speculative verify step vs plain decode step, synthetic 7B shape, {a.layers} layers, GEMV layout; ms per replay, "
          f"median [min, max] of {REPEATS} x {STEPS} replays")
    for batch in a.batches:
        lm, blocks, gen = bdm.build_model(a.layers, max(contexts) + STEPS + 64, dev, "gemv")
        dec = GraphedDecoder(lm, batch=batch)
        for blk in blocks:
            blk.attn.cache.k.normal_(generator=gen)
            blk.attn.cache.v.normal_(generator=gen)
        tok = torch.randint(0, bdm.V, (batch, 8), device=dev, generator=gen)
        for ctx in contexts:
            dec.seek_rows([ctx] * batch)   # per-row positions for both sides: what a speculative run replaces
            dec.step(tok[:, :1])
            plain = timed(dec.stream, dec.replay, reset=lambda: dec.seek_rows([ctx] * batch))
            print(f"batch {batch} context {ctx}: plain step (per-row graph) {plain[0]:.3f} [{plain[1]:.3f}, {plain[2]:.3f}] ms")
            for T in Ts:
                dec.seek_rows([ctx] * batch)
                dec.verify(tok[:, :T])
                graph = dec.verify_graphs[(dec.bucket(ctx + T), T)][0]
                ver = timed(dec.stream, graph.replay)
                # the tail of a full speculative replay on the same logits: argmax of B * T rows + accept + draft
                st = dec._spec_state(T)
                st["params"].copy_(ops.spec_params(max_new_tokens=1 << 30, ngram_max=3))
                st["n_hist"].fill_(200)
                logits = dec.verify_graphs[(dec.bucket(ctx + T), T)][1]

                def tail():
                    dec._spec_tail(st, logits)
                    ops.spec_accept(st["params"], st["tok"], st["pred"], st["hist"], st["n_hist"], st["cnt"], st["ring"],
                                    st["finished"], st["n_hist"].clone(), st["n_hist"].clone(), status=st["status"], steps=st["steps"])
                    ops.ngram_draft(st["params"], st["tok"], st["hist"], st["n_hist"])
                    st["n_hist"].fill_(200)
                    st["cnt"].zero_()
                tl = timed(dec.stream, tail)
                print(f"batch {batch} context {ctx} T {T}: verify step {ver[0]:.3f} [{ver[1]:.3f}, {ver[2]:.3f}] ms, ratio to plain "
                      f"{ver[0] / plain[0]:.2f} (tokens per step to break even); eager argmax + accept + draft launches "
                      f"{tl[0] * 1e3:.0f} us (host-issued: an upper bound of their share of a graph replay)", flush=True)
        del dec, lm, blocks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
