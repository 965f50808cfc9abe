#!/usr/bin/env python3
"""Generates tests/golden/route_a_calls.npz: every call the UNMODIFIED reference modules make into the `awq_ext` / `awq_v2_ext`
shims (function name, positional arguments, keyword arguments) together with the oracle-backed result, the back-end functions
(`autoawq_amd.ops`) the call reached and the test below that issued it.  The tests below run the reference's own
`WQLinear_GEMM / _GEMV / _GEMVFast`, `QuantFusedMLP`, `apply_moe_weights` and `FasterTransformerRMSNorm` code over the shims with
the CPU oracle as back end; they need the reference tree (AutoAWQ's sources, the `awq` package), which is not part of this
repository, so only this script runs them:

    AWQ_REFERENCE_TREE=<AutoAWQ source tree> python tests/golden/make_route_a_calls.py

tests/test_route_a.py replays the recorded calls on the oracle-backed shims (CPU), tests/test_gpu_route_a_replay.py on the HIP
kernels -- VERDICT r05 item 7.

Call sites covered (reference file:line): awq/modules/linear/gemm.py:51-58,100-102 (gemm_forward_cuda, dequantize_weights_cuda
forward and backward), gemv.py:168-180 (gemv_forward_cuda, gemmv2_forward_cuda), gemv_fast.py:191-206 (gemv_forward_cuda_decode,
gemm_forward_cuda_prefill), fused/mlp.py:37-62 (gemm_forward_cuda with five positional arguments), fused/moe.py:60-89,129-133
(grouped_gemm_forward, silu_and_mul, moe_alig_block_size), fused/norm.py:33-36 (layernorm_forward_cuda)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

from conftest import golden  # noqa: E402
from test_route_a import _close, _t, install_oracle_ops  # noqa: E402

REF = os.environ.get("AWQ_REFERENCE_TREE", "")
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "awq")), reason="AWQ_REFERENCE_TREE does not name a reference tree")


# ---- recording mode (main() sets RECORD to a list): the positional call forms of the reference, with their inputs, the oracle-backed
# results and the back-end calls they reached, for tests/test_route_a.py and tests/test_gpu_route_a_replay.py
RECORD = None


def _recording(mname, fname, fn, calls, test):
    def wrapped(*args, **kwargs):
        before = [a.detach().clone() if torch.is_tensor(a) else a for a in args]
        n0 = len(calls)
        ret = fn(*args, **kwargs)
        after = {i: a.detach().clone() for i, a in enumerate(args)
                 if torch.is_tensor(a) and (a.shape != before[i].shape or not torch.equal(a, before[i]))}
        RECORD.append(dict(mod=mname, fn=fname, args=before, kwargs=dict(kwargs), ret=ret.detach().clone() if torch.is_tensor(ret) else ret,
                           mutated=after, test=test, ops=calls[n0:]))
        return ret
    return wrapped


@pytest.fixture()
def route_a(oracle, monkeypatch, request):
    """shims registered as `awq_ext` / `awq_v2_ext`, ops -> oracle, a fresh import of the reference package"""
    from autoawq_amd import awq_ext, awq_v2_ext

    calls = install_oracle_ops(oracle, monkeypatch)
    saved = {k: v for k, v in sys.modules.items() if k == "awq" or k.startswith("awq.") or k in ("awq_ext", "awq_v2_ext")}
    for k in saved:
        del sys.modules[k]
    if RECORD is not None:  # recording mode: every shim call, as the UNMODIFIED reference issues it, goes into the fixture file
        for mod, mname in ((awq_ext, "awq_ext"), (awq_v2_ext, "awq_v2_ext")):
            for fname in [n for n in dir(mod) if callable(getattr(mod, n)) and not n.startswith("_") and getattr(getattr(mod, n), "__module__", "") == mod.__name__]:
                if fname in ("infer_group_size",):
                    continue
                monkeypatch.setattr(mod, fname, _recording(mname, fname, getattr(mod, fname), calls, request.node.name))
    monkeypatch.setitem(sys.modules, "awq_ext", awq_ext)
    monkeypatch.setitem(sys.modules, "awq_v2_ext", awq_v2_ext)
    monkeypatch.syspath_prepend(REF)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    import awq.modules.linear.gemm as rg
    import awq.modules.linear.gemv as rv
    import awq.modules.linear.gemv_fast as rf

    assert rg.awq_ext is awq_ext and rv.awq_ext is awq_ext and rf.awq_v2_ext is awq_v2_ext  # what try_import found
    yield dict(gemm=rg, gemv=rv, fast=rf, calls=calls)
    for k in [k for k in sys.modules if k == "awq" or k.startswith("awq.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_reference_linear_modules_run_on_the_shims(route_a, oracle):
    g = golden("packed_K512_N64_g128")
    K, N, gs = 512, 64, 128
    x = _t(g["x"])                                   # [4, 512] fp16
    W = g["W"]
    bias = _t(g["bias"])
    y32, _ = oracle.matmul(g["x"], W, g["bias"])
    # ---- WQLinear_GEMM: decode branch (gemm_forward_cuda), >= 1024 tokens (dequantize_weights_cuda + matmul), backward
    m = route_a["gemm"].WQLinear_GEMM(4, gs, K, N, True, "cpu")
    m.qweight, m.qzeros, m.scales, m.bias = _t(g["gemm_qweight"]), _t(g["gemm_qzeros"]), _t(g["gemm_scales"]), bias
    out = m(x.view(1, 4, K))
    assert out.shape == (1, 4, N) and _close(out[0].numpy(), y32) and route_a["calls"][-1] == "gemm_forward"
    big = torch.randn((2, 600, K), generator=torch.Generator().manual_seed(0)).half()
    ob = m(big)
    yb, _ = oracle.matmul(big.reshape(-1, K).numpy(), W, g["bias"])
    assert route_a["calls"][-1] == "dequantize_weights" and _close(ob.reshape(-1, N).numpy(), yb)
    mt = route_a["gemm"].WQLinear_GEMM(4, gs, K, N, False, "cpu", training=True)
    mt.qweight, mt.qzeros, mt.scales = m.qweight, m.qzeros, m.scales
    xin = x.view(1, 4, K).clone().requires_grad_(True)
    mt(xin).float().sum().backward()                # backward: dequantize_weights_cuda(qweight, scales, qzeros, 1, 0, 0, False)
    assert _close(xin.grad[0].float().numpy(), np.broadcast_to(W.astype(np.float32).sum(1), (4, K)), ulps=16)
    # ---- WQLinear_GEMV: <= 8 rows (gemv_forward_cuda), > 8 rows (gemmv2_forward_cuda)
    v = route_a["gemv"].WQLinear_GEMV(4, gs, K, N, True, "cpu")
    v.qweight, v.qzeros, v.scales, v.bias = _t(g["gemv_qweight"]), _t(g["gemv_qzeros"]), _t(g["gemv_scales"]), bias
    assert _close(v(x).numpy(), y32) and route_a["calls"][-1] == "gemv_forward"
    x12 = torch.randn((12, K), generator=torch.Generator().manual_seed(1)).half()
    y12, _ = oracle.matmul(x12.numpy(), W, g["bias"])
    assert _close(v(x12).numpy(), y12)
    # ---- WQLinear_GEMVFast: decode (gemv_forward_cuda_decode), prefill (gemm_forward_cuda_prefill: g inferred)
    f = route_a["fast"].WQLinear_GEMVFast(4, gs, K, N, True, "cpu")
    f.qweight, f.qzeros, f.scales, f.bias = _t(g["fast_qweight"]), _t(g["fast_qzeros"]), _t(g["fast_scales"]), bias
    Wf = oracle.dequant_gemvfast(g["fast_qweight"], g["fast_scales"], g["fast_qzeros"], gs)
    yf, _ = oracle.matmul(g["x"], Wf, g["bias"])
    od = f(x.view(4, 1, K))
    assert od.shape == (4, 1, N) and _close(od[:, 0].numpy(), yf) and route_a["calls"][-1] == "gemv_fast_forward"
    op = f(x.view(1, 4, K))
    assert op.shape == (1, 4, N) and _close(op[0].numpy(), yf)
    g64 = golden("packed_K256_N32_g64")              # a g = 64 GEMVFast module: the prefill shim must not assume 128
    f64 = route_a["fast"].WQLinear_GEMVFast(4, 64, 256, 32, False, "cpu")
    f64.qweight, f64.qzeros, f64.scales = _t(g64["fast_qweight"]), _t(g64["fast_qzeros"]), _t(g64["fast_scales"])
    W64 = oracle.dequant_gemvfast(g64["fast_qweight"], g64["fast_scales"], g64["fast_qzeros"], 64)
    y64, _ = oracle.matmul(g64["x"], W64)
    assert _close(f64(_t(g64["x"]).unsqueeze(0))[0].numpy(), y64)


def test_reference_fused_mlp_moe_and_norm_run_on_the_shims(route_a, oracle):
    import awq.modules.fused.mlp as rmlp
    import awq.modules.fused.moe as rmoe
    import awq.modules.fused.norm as rnorm
    from autoawq_amd import awq_ext

    assert rmlp.AWQ_INSTALLED and rmoe.AWQ_INSTALLED and rmoe.awq_ext is awq_ext
    gen = torch.Generator().manual_seed(3)
    H, I, gs, M = 256, 128, 128, 3                   # small: the expert stacks are stored in the fixture, and random int4 words do not compress

    def rand_mod(K, N):
        m = route_a["gemm"].WQLinear_GEMM(4, gs, K, N, False, "cpu")
        m.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, N // 8), dtype=torch.int32, generator=gen)
        m.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // gs, N // 8), dtype=torch.int32, generator=gen)
        m.scales = (torch.rand((K // gs, N), generator=gen) * 0.02 + 0.005).half()
        return m, oracle.dequant_gemm(m.qweight.numpy(), m.qzeros.numpy(), m.scales.numpy(), gs)

    (gate, Wg), (down, Wd), (up, Wu) = rand_mod(H, I), rand_mod(I, H), rand_mod(H, I)
    mlp = rmlp.QuantFusedMLP(gate, down, up)         # self.linear = awq_ext.gemm_forward_cuda, 5th positional arg = 8
    x = torch.randn((1, M, H), generator=gen).half()
    out = mlp(x)
    g16, u16 = oracle.matmul(x[0].numpy(), Wg)[1], oracle.matmul(x[0].numpy(), Wu)[1]
    act = torch.nn.functional.silu(_t(g16)) * _t(u16)
    want, _ = oracle.matmul(act.numpy(), Wd)
    assert out.shape == (1, M, H) and _close(out[0].numpy(), want, ulps=8)
    # ---- apply_moe_weights: moe_alig_block_size fills the caller's tensors, grouped_gemm_forward x2, silu_and_mul(out, gate_up)
    E, T, topk = 4, 5, 2

    class Stack:
        pass
    w1, w2 = Stack(), Stack()
    exps = [(rand_mod(H, 2 * I), rand_mod(I, H)) for _ in range(E)]
    for dst, idx in ((w1, 0), (w2, 1)):
        dst.qweight = torch.stack([e[idx][0].qweight for e in exps])
        dst.qzeros = torch.stack([e[idx][0].qzeros for e in exps])
        dst.scales = torch.stack([e[idx][0].scales for e in exps])
    xt = torch.randn((T, H), generator=gen).half()
    logits = torch.randn((T, E), generator=gen)
    got = rmoe.apply_moe_weights(w1, w2, xt, logits, topk, renormalize=True)
    want, _, _ = oracle.moe_forward(xt.numpy(), logits.numpy(), dict(qweight=w1.qweight.numpy(), qzeros=w1.qzeros.numpy(), scales=w1.scales.numpy()),
                                    dict(qweight=w2.qweight.numpy(), qzeros=w2.qzeros.numpy(), scales=w2.scales.numpy()), topk, gs)
    assert got.shape == (T, H) and _close(got.numpy(), want.astype(np.float32), ulps=8)
    assert {"grouped_gemm_forward", "silu_and_mul"} <= set(route_a["calls"])
    # ---- FasterTransformerRMSNorm.forward: layernorm_forward_cuda(x, weight, out, eps) writes the caller's tensor
    w = (torch.rand(H, generator=gen) + 0.5).half()
    n = rnorm.FasterTransformerRMSNorm(w, 1e-5)
    if not rnorm.IPEX_INSTALLED:
        y = n(x)
        xf = x.float()
        ref = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * w.float())
        assert torch.allclose(y.float(), ref, rtol=2e-3, atol=2e-3) and route_a["calls"][-1] == "rmsnorm"


def main():
    import make_route_a_calls as live  # the module pytest collects below (this file run as a script is __main__)

    assert os.path.isdir(os.path.join(REF, "awq")), "set AWQ_REFERENCE_TREE to the reference's source tree"
    live.RECORD = []
    rc = pytest.main(["-q", "-x", "-p", "no:cacheprovider", "--rootdir", os.path.dirname(TESTS), os.path.abspath(__file__)])
    assert rc == 0, "the reference modules must pass on the shims while their calls are recorded"
    calls = live.RECORD
    arrays, manifest = {}, []

    # content -> key: a tensor several calls pass (the same module's weights) is stored once, and one that is an array of another
    # golden file (the linear modules' packed weights) as "<file>:<name>" (test_route_a.fixture_array reads it from there)
    stored = {}
    for f in ("packed_K512_N64_g128", "packed_K256_N32_g64"):
        for k, a in golden(f).items():
            stored.setdefault((a.dtype.str, a.shape, a.tobytes()), f"{f}:{k}")

    def put(key, t):
        a = t.numpy() if t.dtype != torch.bfloat16 else t.float().numpy()
        key = stored.setdefault((a.dtype.str, a.shape, a.tobytes()), key)
        if ":" not in key:
            arrays[key] = a
        return {"t": key, "dtype": str(t.dtype).replace("torch.", "")}

    for i, c in enumerate(calls):
        e = {"mod": c["mod"], "fn": c["fn"], "test": c["test"], "ops": c["ops"], "args": [], "kwargs": {k: (v if not torch.is_tensor(v) else None) for k, v in c["kwargs"].items()}}
        for j, a in enumerate(c["args"]):
            if torch.is_tensor(a):
                e["args"].append(put(f"c{i}_a{j}", a))
            elif a is None:
                e["args"].append({"none": True})
            else:
                e["args"].append({"v": a if isinstance(a, (bool, int, float)) else float(a)})
        e["ret"] = put(f"c{i}_ret", c["ret"]) if torch.is_tensor(c["ret"]) else None
        e["mutated"] = {str(j): put(f"c{i}_m{j}", t) for j, t in c["mutated"].items()}
        manifest.append(e)
    arrays["manifest"] = np.frombuffer(json.dumps(manifest).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "route_a_calls.npz")
    np.savez_compressed(out, **arrays)
    by = {}
    for e in manifest:
        by[e["mod"] + "." + e["fn"]] = by.get(e["mod"] + "." + e["fn"], 0) + 1
    print(f"{len(manifest)} calls -> {out} ({os.path.getsize(out) / 1e6:.2f} MB):", by)


if __name__ == "__main__":
    main()
