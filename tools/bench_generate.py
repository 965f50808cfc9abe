#!/usr/bin/env python3
"""Token generation on the synthetic Llama-2-7B-shape model of tools/bench_decode_model.py: GraphedDecoder.generate (the
sampler captured into the decode graph, the host looking at the flags every 16 tokens) against the loop users write by hand
(dec.step + torch.argmax + a per-token .item() EOS check), at several contexts and batch sizes.  Decode tok/s excludes the
prompt's prefill (timed on its own and subtracted).  --ragged: prompts of different lengths (attention_mask) in one generate
call, against the same prompts one at a time and a uniform batch padded to the longest prompt.  --sampler-only times the sampler alone (run it under
`rocprofv3 --kernel-trace --stats` for per-kernel durations).  --repetition-penalty / --min-new-tokens add legs with the
sampler's logit processors beside the default ones (in --sampler-only, a history pre-seeded with 2048 ids)."""
import argparse, json, os, sys, time
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def _proc_tag(rp, mnt):
    return f" rp={rp:g} mnt={mnt}"


def bench_generate(layers=32, contexts=(64, 2048), batches=(1, 4), new=128, rp=1.0, mnt=0, kv_cache_dtype="fp16"):
    import bench_decode_model
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    dev = torch.device("cuda")
    lm, blocks, gen = bench_decode_model.build_model(layers, max(contexts) + new + 8, dev, layout="gemv", kv_cache_dtype=kv_cache_dtype)
    V = bench_decode_model.V
    rows = []
    for B in batches:
        dec = GraphedDecoder(lm, batch=B)
        for ctx in contexts:
            prompt = torch.randint(0, V, (B, ctx), device=dev, generator=gen)
            dec.prefill(prompt)  # warm-up (lazy buffers)
            t_pre = min(_timed(lambda: dec.prefill(prompt))[0] for _ in range(2))

            def hand():
                logits = dec.prefill(prompt)
                for _ in range(new - 1):
                    tok = torch.argmax(logits[:, -1], -1)
                    if (tok == -1).any().item():  # the EOS check: a host round trip per token
                        break
                    logits = dec.step(tok)
                return torch.argmax(logits[:, -1], -1)

            cfgs = [("hand greedy", hand), ("generate greedy", lambda: dec.generate(prompt, new)),
                    ("generate top_k=50 top_p=0.9", lambda: dec.generate(prompt, new, do_sample=True, top_k=50, top_p=0.9, seed=1))]
            if rp != 1.0 or mnt:
                proc = {"repetition_penalty": rp, "min_new_tokens": mnt}
                cfgs += [("generate greedy" + _proc_tag(rp, mnt), lambda: dec.generate(prompt, new, **proc)),
                         ("generate top_k=50 top_p=0.9" + _proc_tag(rp, mnt),
                          lambda: dec.generate(prompt, new, do_sample=True, top_k=50, top_p=0.9, seed=1, **proc))]
            for name, fn in cfgs:
                fn()  # captures
                t = min(_timed(fn)[0] for _ in range(2))
                dt = max(t - t_pre, 1e-9)
                r = {"batch": B, "context": ctx, "mode": name, "new_tokens": new, "total_s": round(t, 5), "prefill_s": round(t_pre, 5),
                     "decode_tok_s": round(B * (new - 1) / dt, 1)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        del dec
    return rows


def _left_padded(prompts, dev):
    S = max(p.shape[0] for p in prompts)
    ids = torch.zeros((len(prompts), S), dtype=torch.int64, device=dev)
    mask = torch.zeros_like(ids)
    for b, p in enumerate(prompts):
        ids[b, S - p.shape[0]:] = p
        mask[b, S - p.shape[0]:] = 1
    return ids, mask


def bench_ragged(layers=32, batches=(4, 8), new=128, shortest=64, longest=2048, kv_cache_dtype="fp16"):
    """Prompts spread evenly between `shortest` and `longest` tokens.  'ragged' = one generate call with the attention_mask
    (per-row positions); 'one at a time' = each prompt through a batch-1 decoder, times summed; 'uniform padded' = the padded
    batch without a mask (every row at the longest context: what per-row lengths save -- its tokens are NOT correct for the
    shorter prompts).  Greedy; decode tok/s = batch * (new - 1) / (total - prefill)."""
    import bench_decode_model
    from autoawq_amd.modules.fused.decode import GraphedDecoder

    dev = torch.device("cuda")
    lm, blocks, gen = bench_decode_model.build_model(layers, longest + new + 8, dev, layout="gemv", kv_cache_dtype=kv_cache_dtype)
    V = bench_decode_model.V
    rows = []

    def leg(B, name, lengths, runs):
        """runs: [(prefill fn, generate fn)], timed one after the other and summed"""
        t_pre = t_all = 0.0
        for pre, fn in runs:
            fn()  # warm-up and captures
            t_pre += min(_timed(pre)[0] for _ in range(2))
            t_all += min(_timed(fn)[0] for _ in range(2))
        r = {"batch": B, "lengths": lengths, "mode": name, "new_tokens": new, "total_s": round(t_all, 5), "prefill_s": round(t_pre, 5),
             "decode_tok_s": round(B * (new - 1) / max(t_all - t_pre, 1e-9), 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)

    for B in batches:
        lengths = [int(round(shortest + (longest - shortest) * i / (B - 1))) for i in range(B)]
        prompts = [torch.randint(0, V, (n,), device=dev, generator=gen) for n in lengths]
        ids, mask = _left_padded(prompts, dev)
        dec = GraphedDecoder(lm, batch=B)
        leg(B, "ragged", lengths, [(lambda: dec.prefill(ids, attention_mask=mask), lambda: dec.generate(ids, new, attention_mask=mask))])
        leg(B, "uniform padded", [longest] * B, [(lambda: dec.prefill(ids), lambda: dec.generate(ids, new))])
        del dec
        dec = GraphedDecoder(lm, batch=1)
        leg(B, "one at a time", lengths, [((lambda p=p: dec.prefill(p.view(1, -1))), (lambda p=p: dec.generate(p.view(1, -1), new)))
                                          for p in prompts])
        del dec
    return rows


def bench_sampler(vocabs=(32000, 128256, 152064), batches=(1, 4), calls=200, rp=1.0, mnt=0):
    from autoawq_amd import ops

    dev = torch.device("cuda")
    rows = []
    for V in vocabs:
        for B in batches:
            x = (torch.randn((B, V), device=dev) * 3).half()
            t = torch.ones(1, dtype=torch.int32, device=dev)
            out = torch.empty(B, dtype=torch.int64, device=dev)
            status = torch.zeros((B + 31) // 32, dtype=torch.int32, device=dev)
            ws = torch.zeros(ops.sample_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
            legs = [(False, "greedy", True, {"do_sample": False}),
                    (False, "top_k=50 top_p=0.9", False, {"do_sample": True, "top_k": 50, "top_p": 0.9, "seed": 1}),
                    (False, "top_p=0.9", False, {"do_sample": True, "top_p": 0.9, "seed": 1})]
            if rp != 1.0 or mnt:
                legs += [(True, name + _proc_tag(rp, mnt), greedy, cfg) for _, name, greedy, cfg in legs]
            for proc_on, name, greedy, cfg in legs:
                params = ops.sample_params(eos_ids=[V - 1] if proc_on else (), **cfg).to(dev)
                proc = hist = None
                if proc_on:  # the history of a 2048-token context
                    proc = ops.sample_proc_params(rp, mnt).to(dev)
                    hist = ops.sample_history(torch.randint(0, V, (B, 2048), device=dev), V)
                launch = lambda: ops.sample_launch(x, params, t, out, status, ws, greedy=greedy, proc=proc, history=hist)
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    launch()
                    s.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s):
                        for _ in range(10):
                            launch()
                    g.replay()
                    s.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(calls // 10):
                        g.replay()
                    e1.record(s)
                    e1.synchronize()
                us = e0.elapsed_time(e1) * 1000.0 / calls
                assert int(status.count_nonzero()) == 0 and int(ws.count_nonzero()) == 0
                r = {"V": V, "batch": B, "mode": name, "us_per_call_in_graph": round(us, 2)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler-only", action="store_true")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--min-new-tokens", type=int, default=0)
    ap.add_argument("--kv-cache-dtype", choices=["fp16", "fp8"], default="fp16")
    a = ap.parse_args()
    if a.sampler_only:
        bench_sampler(rp=a.repetition_penalty, mnt=a.min_new_tokens)
    elif a.ragged:
        bench_ragged(layers=a.layers, new=a.new, kv_cache_dtype=a.kv_cache_dtype)
    else:
        bench_generate(layers=a.layers, new=a.new, rp=a.repetition_penalty, mnt=a.min_new_tokens, kv_cache_dtype=a.kv_cache_dtype)
