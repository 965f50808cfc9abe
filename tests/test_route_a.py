"""Route A: the UNMODIFIED reference modules' calls into the `awq_ext` / `awq_v2_ext` shims, on CPU.

tests/golden/route_a_calls.npz holds every call the reference's own `WQLinear_GEMM / _GEMV / _GEMVFast`, `QuantFusedMLP`,
`apply_moe_weights` and `FasterTransformerRMSNorm` code made into the shims -- ITS positional argument orders and return
conventions, every call site of SURVEY.md section 2.2 -- recorded by tests/golden/make_route_a_calls.py while those modules ran over
the shims with the shims' back end (`autoawq_amd.ops`) replaced by the CPU oracle (test infrastructure may use it; the product
never does).  Here each call is replayed on the same oracle-backed shims: it must reach the same back-end functions and return,
and write into its arguments, what it did when the reference issued it.  The same calls are replayed on the HIP kernels by
tests/test_gpu_route_a_replay.py."""
import json
import os

import numpy as np
import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_a_calls.npz")
BIT_EXACT = {"dequantize_weights_cuda", "moe_alig_block_size"}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def fixture_array(d, key):
    """array `key` of the loaded fixture `d`; "<file>:<name>" is array <name> of tests/golden/<file>.npz (not stored twice)"""
    if ":" in key:
        f, name = key.split(":")
        return np.load(os.path.join(os.path.dirname(FIXTURE), f + ".npz"))[name]
    return d[key]


def install_oracle_ops(oracle, monkeypatch):
    """ops -> oracle for the shims; returns the list every back-end call appends its name to"""
    from autoawq_amd import ops

    calls = []

    def dequantize_weights(qweight, scales, qzeros):
        calls.append("dequantize_weights")
        G = qzeros.shape[0]
        return _t(oracle.dequant_gemm(qweight.numpy(), qzeros.numpy(), scales.numpy(), qweight.shape[0] // G))

    def gemm_forward(x2d, qweight, scales, qzeros, bias=None, flags=0):
        calls.append("gemm_forward")
        g = qweight.shape[0] // qzeros.shape[0]
        _, y16 = oracle.linear_gemm(x2d.numpy(), qweight.numpy(), qzeros.numpy(), scales.numpy(), g)
        return _t(y16)

    def gemv_forward(x2d, qweight, scales, qzeros, group_size, flags=0):
        calls.append("gemv_forward")
        W = oracle.dequant_gemv(qweight.numpy(), qzeros.numpy(), scales.numpy(), group_size)
        return _t(oracle.matmul(x2d.numpy(), W)[1])

    def gemv_fast_forward(x2d, qweight, scales, qzeros, group_size, flags=0):
        calls.append("gemv_fast_forward")
        W = oracle.dequant_gemvfast(qweight.numpy(), scales.numpy(), qzeros.numpy(), group_size)
        return _t(oracle.matmul(x2d.numpy(), W)[1])

    def dequantize_weights_gemv_fast(qweight, scales, qzeros, group_size):
        calls.append("dequantize_weights_gemv_fast")
        return _t(np.ascontiguousarray(oracle.dequant_gemvfast(qweight.numpy(), scales.numpy(), qzeros.numpy(), group_size).T))

    def silu_and_mul(gate_up, out=None):
        calls.append("silu_and_mul")
        r = _t(oracle.silu_and_mul(gate_up.numpy()))
        if out is None:
            return r
        out.copy_(r)
        return out

    def rmsnorm(x, weight, eps, residual=None, out=None):
        calls.append("rmsnorm")
        xf = x.float()
        r = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()).to(x.dtype)
        if out is None:
            return r
        out.copy_(r)
        return out

    def grouped_gemm_forward(x, qweight, scales, qzeros, topk_weights, sorted_token_ids, expert_ids, num_tokens_post_padded,
                             mul_weights, split_k_iters=8, block_rows=16):
        calls.append("grouped_gemm_forward")
        T, topk = topk_weights.shape
        E, K, NW = qweight.shape
        g = K // qzeros.shape[1]
        x2 = x.reshape(-1, K)
        x_div = topk if x.shape[1] == 1 else 1
        y = torch.zeros((T * topk, NW * 8), dtype=torch.float16)
        npad = int(num_tokens_post_padded.reshape(-1)[0])
        for blk in range(npad // block_rows):
            e = int(expert_ids[blk])
            for r in range(block_rows):
                pid = int(sorted_token_ids[blk * block_rows + r])
                if pid >= T * topk:
                    continue
                y32, _ = oracle.linear_gemm(x2[pid // x_div: pid // x_div + 1].numpy(), qweight[e].numpy(), qzeros[e].numpy(),
                                            scales[e].numpy(), g)
                row = _t(y32)[0]
                if mul_weights:
                    row = row * float(topk_weights.reshape(-1)[pid])
                y[pid] = row.half()
        return y.reshape(T, topk, NW * 8)

    for name, fn in dict(dequantize_weights=dequantize_weights, gemm_forward=gemm_forward, gemv_forward=gemv_forward,
                         gemv_fast_forward=gemv_fast_forward, dequantize_weights_gemv_fast=dequantize_weights_gemv_fast,
                         silu_and_mul=silu_and_mul, rmsnorm=rmsnorm, grouped_gemm_forward=grouped_gemm_forward).items():
        monkeypatch.setattr(ops, name, fn)
    return calls


def _close(y, ref32, ulps=4):
    y, ref32 = np.asarray(y, np.float64), np.asarray(ref32, np.float64)
    rms = float(np.sqrt(np.mean(ref32 ** 2))) if ref32.size else 0.0
    tol = ulps * np.maximum(np.abs(ref32), 2.0 ** -14) * 2.0 ** -10 + 2e-3 * np.abs(ref32) + 2e-3 * rms
    return bool((np.abs(y - ref32) <= tol).all())


def _replay(test, oracle, monkeypatch, ulps):
    """every recorded call that `test` (of tests/golden/make_route_a_calls.py) issued, replayed on the oracle-backed shims"""
    from autoawq_amd import awq_ext, awq_v2_ext

    calls = install_oracle_ops(oracle, monkeypatch)
    d = np.load(FIXTURE)
    entries = [e for e in json.loads(bytes(d["manifest"]).decode()) if e["test"] == test]
    assert entries, f"{test}: no recorded calls"
    for e in entries:
        args = []
        for a in e["args"]:
            if "t" in a:
                args.append(_t(fixture_array(d, a["t"])).to(getattr(torch, a["dtype"])))
            elif "none" in a:
                args.append(None)
            else:
                args.append(a["v"])
        calls.clear()
        ret = getattr({"awq_ext": awq_ext, "awq_v2_ext": awq_v2_ext}[e["mod"]], e["fn"])(*args, **{k: v for k, v in e["kwargs"].items() if v is not None})
        what = f'{e["mod"]}.{e["fn"]} ({len(e["args"])} positional arguments)'
        assert calls == e["ops"], f"{what}: reached {calls}, the reference's call reached {e['ops']}"
        pairs = []
        if e["ret"] is not None:
            assert torch.is_tensor(ret), f"{what}: the reference expects a tensor back"
            pairs.append((ret, fixture_array(d, e["ret"]["t"]), "return value"))
        for j, m in e["mutated"].items():
            pairs.append((args[int(j)], fixture_array(d, m["t"]), f"argument {j} (written by the call)"))
        assert pairs, f"{what}: nothing to compare"
        for got, want, name in pairs:
            assert tuple(got.shape) == tuple(want.shape), (what, name, tuple(got.shape), want.shape)
            g = got.float().numpy() if got.dtype == torch.bfloat16 else got.numpy()
            if e["fn"] in BIT_EXACT or not np.issubdtype(want.dtype, np.floating):
                assert np.array_equal(g, want), f"{what}: {name} differs from the reference-side result"
            else:
                assert _close(g, want, ulps), f"{what}: {name} outside tolerance (max err {np.abs(g.astype(np.float64) - want).max()})"
    return entries


def test_reference_linear_modules_run_on_the_shims(oracle, monkeypatch):
    # WQLinear_GEMM: decode branch (gemm_forward_cuda), >= 1024 tokens (dequantize_weights_cuda + matmul), backward
    # (dequantize_weights_cuda(qweight, scales, qzeros, 1, 0, 0, False)); WQLinear_GEMV: <= 8 rows (gemv_forward_cuda), > 8 rows
    # (gemmv2_forward_cuda); WQLinear_GEMVFast: decode (gemv_forward_cuda_decode), prefill (gemm_forward_cuda_prefill: g inferred),
    # a g = 64 module among them (the prefill shim must not assume 128)
    entries = _replay("test_reference_linear_modules_run_on_the_shims", oracle, monkeypatch, ulps=4)
    assert {e["mod"] + "." + e["fn"] for e in entries} >= {
        "awq_ext.gemm_forward_cuda", "awq_ext.dequantize_weights_cuda", "awq_ext.gemv_forward_cuda", "awq_ext.gemmv2_forward_cuda",
        "awq_v2_ext.gemv_forward_cuda_decode", "awq_v2_ext.gemm_forward_cuda_prefill"}
    assert any(e["fn"] == "dequantize_weights_cuda" and len(e["args"]) == 7 for e in entries)
    assert {e["ops"][-1] for e in entries if e["fn"] == "gemm_forward_cuda"} == {"gemm_forward"}
    assert sum(e["fn"] == "gemm_forward_cuda_prefill" for e in entries) >= 2


def test_reference_fused_mlp_moe_and_norm_run_on_the_shims(oracle, monkeypatch):
    # QuantFusedMLP (gemm_forward_cuda with split_k_iters as the FIFTH positional argument), apply_moe_weights
    # (moe_alig_block_size fills the caller's tensors, grouped_gemm_forward x2, silu_and_mul(out, gate_up)),
    # FasterTransformerRMSNorm.forward (layernorm_forward_cuda(x, weight, out, eps) writes the caller's tensor)
    entries = _replay("test_reference_fused_mlp_moe_and_norm_run_on_the_shims", oracle, monkeypatch, ulps=8)
    assert {e["mod"] + "." + e["fn"] for e in entries} >= {
        "awq_ext.gemm_forward_cuda", "awq_ext.moe_alig_block_size", "awq_ext.grouped_gemm_forward", "awq_ext.silu_and_mul",
        "awq_ext.layernorm_forward_cuda"}
    assert any(e["fn"] == "gemm_forward_cuda" and len(e["args"]) == 5 for e in entries)
    assert {"grouped_gemm_forward", "silu_and_mul", "rmsnorm"} <= {o for e in entries for o in e["ops"]}
