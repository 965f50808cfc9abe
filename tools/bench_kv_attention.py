"""Decode attention at the Llama-2-7B shape, fp16 vs fp8 KV cache (profiles/kv_fp8.txt): ops.decode_attention_rope -- the
per-layer launch GraphedDecoder replays -- alternating the two cache types, device-event timing over 200 launches per point."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from autoawq_amd import ops
from autoawq_amd.modules.fused.attn import RoPE

Hq = Hkv = 32
reps = 200
for B in (1, 8):
    for T in (64, 512, 2048, 8192):
        Tmax = T + 8
        r = RoPE(128, Tmax, "cuda", 10000)
        qkv = torch.randn((B, 1, (Hq + 2 * Hkv) * 128), device="cuda").half()
        res = {}
        k16 = torch.randn((B, Tmax, Hkv, 128), device="cuda").half(); v16 = torch.randn_like(k16)
        k8 = torch.zeros((B, Tmax, Hkv, 128), dtype=torch.uint8, device="cuda"); v8 = torch.zeros_like(k8)
        ks = torch.zeros((B, Tmax, Hkv), device="cuda"); vs = torch.zeros_like(ks)
        ops.kv_quant_fp8(k16, k8, ks); ops.kv_quant_fp8(v16, v8, vs)
        pos = torch.tensor([T - 1], dtype=torch.int32, device="cuda")
        calls = {"fp16": lambda: ops.decode_attention_rope(qkv, k16, v16, r.cos, r.sin, 0, Hq, Hkv, pos_dev=pos, max_len=T),
                 "fp8": lambda: ops.decode_attention_rope(qkv, k8, v8, r.cos, r.sin, 0, Hq, Hkv, pos_dev=pos, max_len=T,
                                                          k_scale=ks, v_scale=vs)}
        times = {"fp16": [], "fp8": []}
        for rnd in range(4):
            for name in ("fp16", "fp8") if rnd % 2 == 0 else ("fp8", "fp16"):
                f = calls[name]
                for _ in range(10):
                    f()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    f()
                e1.record(); e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1000 / reps)
        fp16, fp8 = min(times["fp16"]), min(times["fp8"])
        print(f"bs {B} ctx {T}: decode_attention_rope per launch (incl. combine) fp16 {fp16:.2f} us, fp8 {fp8:.2f} us "
              f"(fp8/fp16 {fp8 / fp16:.3f}); cache bytes per layer read: fp16 {2 * B * T * Hkv * 256 / 1e6:.1f} MB, "
              f"fp8 {2 * B * T * Hkv * 132 / 1e6:.1f} MB; all rounds fp16 {['%.2f' % t for t in times['fp16']]} "
              f"fp8 {['%.2f' % t for t in times['fp8']]}", flush=True)
        del k16, v16, k8, v8, ks, vs
        torch.cuda.empty_cache()
