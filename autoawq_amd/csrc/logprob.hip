// logprob.hip -- log-probability of one token id per row of fp16 logits (awq_token_logprobs, include/awq_hip.h):
//
//     out[r] = (x[id] - m) - log sum_i exp(x_i - m),      x = the row cast to fp32, m = max_i x_i
//
// the model's own distribution: no temperature, no top-k / top-p, no logit processor (what perplexity needs, and what serving
// APIs mean by `logprobs`).  One launch, ONE BLOCK PER ROW, no workspace, no atomics, capturable.  At decode the rows are a few
// hundred KB that lm_head has just written (latency-bound however they are split); sequence scoring has thousands of rows and a
// row per block fills the chip.  tools/bench_logprobs.py times both ends (profiles/token_logprobs.txt).
//
// Geometry (tests/logprob_bound.py restates it): kThreads = 1024 threads, kVec = 8 halves per thread per step, so a step covers
// kStep = 8192 elements and a row takes steps = ceil(V / 8192) of them.
//   * vector path (row base and row stride multiples of 8 elements): thread t of step k owns elements 8192 k + 8 t .. + 7, one
//     16-byte load; the vector that straddles V is read element by element and padded with -inf: no byte past the row's V
//     elements is touched.
//   * element path (any other base or stride, e.g. V = 50257 or a view offset by one element): thread t of step k owns
//     elements 8192 k + 1024 j + t, j = 0 .. 7: eight coalesced 2-byte loads.  Same arithmetic, same depth.
//   * per thread an online (m, s): v = max of the 8 (exact); if v > m: s *= exp(m - v), m = v (ONE rescale per 8-vector); then
//     s += exp(x_j - m), j = 0 .. 7 in order.  9 roundings per step on s.
//   * merge of two partials: M = max(m_a, m_b), s = s_a e_a + s_b e_b with e = 1 where the side's m equals M and exp(m - M)
//     otherwise (one multiply and one add on every term's path, one exp).  6 xor-shuffle levels inside a wave, then wave 0 merges
//     the 16 waves' partials from LDS in 4 more levels.
//   * thread 0: out = (x[id] - m) - logf(s)   (OCML logf), the slot bookkeeping below, plain vector stores.
// Summation depth of a term (adds + rescale multiplies on its path):   N(V)     = 9 ceil(V / 8192) + 2 (6 + 4) = 9 steps + 20.
// exp evaluations on a term's chain (own + rescales + merges):         n_exp(V) = 1 + ceil(V / 8192) + 6 + 4  = steps + 11.
// Every exp is v_exp_f32 of (x - m) log2(e): the difference rounds once, the product with the rounded constant once more.
//
// Contract: -inf logits contribute 0; the id's own logit -inf gives -inf; a row holding NaN or +inf, or all -inf, gives NaN;
// id < 0 is an ignored slot and writes 0.0f (the row is not read); id >= V gives NaN.
// slot != NULL: row r writes out[r * out_stride + slot[r]] (dropped unless 0 <= slot[r] < out_cap) and then slot[r] += 1 -- one
// thread of the row's block does both; slot == NULL: out[r * out_stride].
#include <math.h>

#include "awq_device.h"
#include "awq_internal.h"

namespace {

constexpr int kThreads = 1024, kVec = 8, kStep = kThreads * kVec, kWaves = kThreads / 64;

struct LogprobWords {
    const half_t* logits;
    int64_t logits_stride;
    const int64_t* ids;
    int64_t ids_stride;
    float* out;
    int64_t out_stride;
    int32_t* slot;
    int64_t out_cap;
    int V;
};

AWQ_DEV void merge(float& m, float& s, float mo, float so) {
#pragma clang fp contract(off)
    const float M = fmaxf(m, mo);
    if (M == -INFINITY) return;  // both sides empty: s = 0 stays
    const float ea = m == M ? 1.f : __expf(m - M), eb = mo == M ? 1.f : __expf(mo - M);
    s = s * ea + so * eb;
    m = M;
}

// one 8-vector into the thread's running (m, s); bad: a NaN or +inf was seen
AWQ_DEV void update(const float (&x)[kVec], float& m, float& s, bool& bad) {
#pragma clang fp contract(off)
    float v = x[0];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        bad |= !(x[j] < INFINITY);
        v = fmaxf(v, x[j]);
    }
    if (v > m) {  // (m = -inf, s = 0 at the start: exp(-inf) = 0)
        s *= __expf(m - v);
        m = v;
    }
    if (m == -INFINITY) return;  // nothing but -inf so far: x - m would be NaN
#pragma unroll
    for (int j = 0; j < kVec; ++j) s += __expf(x[j] - m);
}

// VEC: the row's base and stride are multiples of 8 elements (16-byte loads); otherwise the element path
template <bool VEC>
__global__ __launch_bounds__(kThreads) void awq_token_logprobs_kernel(LogprobWords w) {
    __shared__ float sm[kWaves], ss[kWaves];
    __shared__ int sbad;
    const int64_t r = blockIdx.x;
    const int t = threadIdx.x, V = w.V;
    const int64_t id = w.ids[r * w.ids_stride];
    const half_t* x = w.logits + r * w.logits_stride;
    float m = -INFINITY, s = 0.f;
    bool bad = false;
    if (id >= 0) {  // (uniform over the block; an ignored slot reads nothing of its row)
        const int full = V / kStep;  // steps in which every thread owns 8 elements inside the row
        float f[kVec];
#pragma unroll 2
        for (int k = 0; k < full; ++k) {
            if constexpr (VEC) {
                const half8_t h = *reinterpret_cast<const half8_t*>(x + (int64_t)k * kStep + t * kVec);
#pragma unroll
                for (int j = 0; j < kVec; ++j) f[j] = (float)h[j];
            } else {
#pragma unroll
                for (int j = 0; j < kVec; ++j) f[j] = (float)x[(int64_t)k * kStep + j * kThreads + t];
            }
            update(f, m, s, bad);
        }
        const int base = full * kStep;
        if (base < V) {  // the last, partial step: elements at and past V are -inf and never loaded
            bool any = false;
            if constexpr (VEC) {
                const int e0 = base + t * kVec;
                if (e0 + kVec <= V) {
                    const half8_t h = *reinterpret_cast<const half8_t*>(x + e0);
#pragma unroll
                    for (int j = 0; j < kVec; ++j) f[j] = (float)h[j];
                    any = true;
                } else {
#pragma unroll
                    for (int j = 0; j < kVec; ++j) {
                        f[j] = e0 + j < V ? (float)x[e0 + j] : -INFINITY;
                    }
                    any = e0 < V;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kVec; ++j) {
                    const int e = base + j * kThreads + t;
                    f[j] = e < V ? (float)x[e] : -INFINITY;
                }
                any = base + t < V;
            }
            if (any) update(f, m, s, bad);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) merge(m, s, __shfl_xor(m, d, 64), __shfl_xor(s, d, 64));
    }
    if (t == 0) sbad = 0;
    __syncthreads();
    if ((t & 63) == 0) sm[t >> 6] = m, ss[t >> 6] = s;
    if (bad) sbad = 1;  // (every writer stores the same word)
    __syncthreads();
    if (t >= 64) return;
    if (id >= 0) {
        m = t < kWaves ? sm[t] : -INFINITY;
        s = t < kWaves ? ss[t] : 0.f;
#pragma unroll
        for (int d = 1; d < kWaves; d <<= 1) merge(m, s, __shfl_xor(m, d, 64), __shfl_xor(s, d, 64));
    }
    if (t != 0) return;
    float y = 0.f;
    if (id >= 0) {
#pragma clang fp contract(off)
        if (id >= V || sbad || m == -INFINITY)
            y = NAN;
        else
            y = ((float)x[id] - m) - logf(s);
    }
    float* o = w.out + r * w.out_stride;
    if (w.slot) {
        const int32_t k = w.slot[r];
        if (k >= 0 && k < w.out_cap) o[k] = y;
        w.slot[r] = k + 1;
    } else {
        *o = y;
    }
}

}  // namespace

int awq_launch_token_logprobs(const AwqLogprobArgs& a) {
    const LogprobWords w{reinterpret_cast<const half_t*>(a.logits), a.logits_stride, a.ids, a.ids_stride, a.out, a.out_stride,
                         a.slot, a.out_cap, (int)a.V};
    // (with one row the stride is never applied)
    const bool vec = (reinterpret_cast<uintptr_t>(a.logits) & 15u) == 0 && (a.R == 1 || a.logits_stride % kVec == 0);
    const dim3 grid((unsigned)a.R), block(kThreads);
    const hipStream_t st = static_cast<hipStream_t>(a.stream);
    if (vec)
        hipLaunchKernelGGL(awq_token_logprobs_kernel<true>, grid, block, 0, st, w);
    else
        hipLaunchKernelGGL(awq_token_logprobs_kernel<false>, grid, block, 0, st, w);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}
