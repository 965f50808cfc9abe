#!/usr/bin/env python3
"""Generates tests/golden/gemv_batch_auto_plans.npz: the AUTO plan (form 0, ring depth 0) of the batched decode kernel
(csrc/gemv_batch.hip) for every M = 1 .. 128 at the benched shapes, both layouts, as awq_gemv_batch_plan reports it.  Recorded
from the planner before it learnt to refuse / clamp empty row parts; tests/test_gemv_batch_plan_cpu.py asserts that the AUTO plans
have stayed identical (the empty-part fix must not change what AUTO runs).  Needs a built libawq_hip.so, no GPU:

    python tests/golden/make_gemv_batch_plans.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (K, N): the four 7B Linears, the four 70B TP = 8 shards, the gemm_bs leg of bench.py (4096 x 11008)
SHAPES = [(4096, 12288), (4096, 4096), (4096, 22016), (11008, 4096), (8192, 1280), (1024, 8192), (8192, 7168), (3584, 8192),
          (4096, 11008)]


def auto_plans(plan):
    """int32 [layout (0 GEMV, 1 GEMVFast), shape, M - 1, field]; every field -1 where AUTO is refused"""
    out = np.full((2, len(SHAPES), 128, 15), -1, np.int32)
    for fast in (0, 1):
        for s, (K, N) in enumerate(SHAPES):
            for M in range(1, 129):
                p = plan(M, K, N, 128, 0, 0, fast)
                if p is not None:
                    out[fast, s, M - 1] = p
    return out


if __name__ == "__main__":
    import ctypes

    from autoawq_amd import _lib

    def plan(M, K, N, g, form, depth, fast):
        buf = (ctypes.c_int32 * 15)()
        rc = _lib.lib().awq_gemv_batch_plan(M, K, N, g, form, depth, fast, buf)
        return list(buf) if rc == 0 else None

    np.savez_compressed(os.path.join(HERE, "gemv_batch_auto_plans.npz"), shapes=np.array(SHAPES, np.int32), plans=auto_plans(plan))
