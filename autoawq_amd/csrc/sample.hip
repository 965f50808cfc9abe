// sample.hip -- on-device token selection from fp16 logits (awq_sample_tokens, include/awq_hip.h).
//
// Contract (pinned by tests/test_sampling_cpu.py and tests/test_gpu_sampling.py):
//   * greedy (do_sample == 0 or temperature <= 0): argmax of the row, ties to the LOWEST index (torch.argmax).
//   * sampling: temperature, then top-k, then top-p -- the order of transformers' `_get_logits_processor`
//     (generation/utils.py: TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper are appended in that order).
//       top_k in 0 (off) or 1..V: keep every token whose logit is >= the k-th largest (boundary ties kept, as
//         TopKLogitsWarper does).
//       top_p in (0, 1], 1 = off: on softmax(logit / T) over the top-k-kept set, tau = the LARGEST logit value such that
//         the tokens with logit >= tau carry mass >= top_p; keep exactly those.  On tie-free rows this is
//         TopPLogitsWarper's set; a tied group at the boundary is kept whole (the warper's stable sort may cut through it).
//       draw: Gumbel-max, token = argmax over kept i of logit_i / T + g_i, g_i = -log(-log(u_i)), ties to the lowest
//         index -- the exact categorical distribution of the kept set, with no sort and no CDF scan.
//   * random numbers: Philox4x64-10 (Salmon et al., SC'11; the constants of Random123 and numpy's np.random.Philox):
//       u_i = word (i % 4) of Philox4x64-10(key = (seed, 0), counter = (t, row, i / 4, 0)), u = ((w >> 41) + 0.5) * 2^-23
//       in fp32 (exact: 0 < u < 1), t = 1-based index of the generated token (a device word the launch itself advances).
//   * -inf logits are legal and never kept.  A row holding NaN or +inf, or one where nothing survives (all -inf), sets its
//     bit in the sticky status words and emits `pad`.
//   * bookkeeping in the same launch: out[row * out_stride] = token (int64: the decoder's input-id buffer),
//     ring[row * ring_cap + t - 1] = token (int32), finished[row] latches once a row emits one of its EOS ids; a finished
//     row is not sampled again and emits `pad`.  The launch's last-arriving row increments *t.
//
// Pipeline.  A row is split into 2048-element chunks, one 256-thread block each (grid = chunks x rows), and every pass ends
// in a last-arriving-block combine per row through the workspace.  fp16 logits map to a monotone 16-bit key (-0 folded into
// +0, so that key order is value order and equal keys are equal values): 65536 values, so two 8-bit radix rounds find any
// threshold exactly.  Masses are exp((logit - max) / T) in fixed point (2^-43 units, u64): integer sums are order-free, so
// the per-bin sums of one pass equal those of the next bit for bit and the result does not depend on block timing.
//   pass 1: max / argmax (packed key:~index, one u64 atomicMax), NaN / +inf flag, high-byte histogram of counts.
//           Greedy: the combine ends the call here.  Sampling: the combine finds the top-k boundary bin.
//   pass 2: low-byte counts and masses of the top-k boundary bin, masses of the bins above it.  The combine fixes the
//           top-k threshold, the kept mass Z and the top-p boundary bin.
//   pass 3: Gumbel scores of the kept tokens: the best above the top-p bin, and per low byte of the top-p bin its best score
//           and mass.  The combine fixes the top-p threshold inside the bin, takes the winner and does the bookkeeping.
// Passes 2 and 3 return at once when the parameters say greedy, so one captured graph serves either configuration.
//
// Logit processors (awq_sample_tokens_ex; pinned by tests/test_sampling_penalty_cpu.py and tests/test_gpu_sampling_penalty.py):
// transformers' RepetitionPenaltyLogitsProcessor then MinNewTokensLengthLogitsProcessor, which `generate` applies to the fp32 cast
// of the logits before the warpers (greedy too).  For row r at token index t (read at block start: the launch's last row
// advances t only after every block of every row has arrived) the logit i with fp16 bits h is processed as
//   1. t <= min_new_tokens and i one of the n_eos EOS ids: h = -inf (new-token count t - 1 < min_new_tokens);
//   2. otherwise, bit i of history row r set and h finite: v = float(h), v = v < 0 ? v * p : v / p in fp32 (the correctly
//      rounded division: no __fdividef / rcp), then fp16 round-to-nearest-even saturating to +-65504 -- a finite logit stays
//      finite (a penalty below 1 cannot make a +inf that would set the status bit), +-0 keep their sign (the key folds them);
//      -inf, +inf and NaN pass unchanged, so the status rules above are unchanged.
//   Every pass, and the greedy argmax, reads the processed value (process8 after each load8): the contract above applied to
//   process(logits).  Tie rule: the processed value is exactly fp16(transformers' fp32 value) wherever that is in range, so the
//   token equals transformers' on rows where no two candidates collide after that rounding (as for the top-p boundary rule).
//   Bookkeeping: finish_row ORs the bit of the token written to out[row] into history row r (every row, the pad of a finished or
//   failed row included, as transformers' input_ids carry it; a pad outside [0, V) sets nothing), after every block of the row
//   has read the history.  awq_sample_history_seed ORs an id matrix into a history (a prompt).
// The PROC = false instantiations are the kernels of awq_sample_tokens, instruction for instruction.
//
// Rows form (awq_sample_tokens_rows, the ROWS template flag; pinned by tests/test_sampling_rows_cpu.py and
// tests/test_gpu_sampling_rows.py): every row is a request of its own.  A block of row r reads params[r], t[r] and (PROC) proc[r]
// -- indexed in device memory, never copied -- and the contract above holds with the row's values: greedy or sampled per row
// (passes 2 and 3 return for a greedy row), Philox key (seed[r], 0) and counter (t[r], r, i / 4, 0), suppression while
// t[r] <= min_new_tokens[r], ring[r * ring_cap + t[r] - 1], the row's EOS ids and pad.  t[r] is advanced by row r's own last
// combine (finish_row), which runs after every block of the row has arrived, i.e. has read t[r]: no launch-wide step, WsHead is
// not touched.  max_new (optional): with max_new[r] > 0 the row latches finished[r] in the launch that emits token index
// t[r] >= max_new[r]; that token is real, the following ones are pad.
// The ROWS = false instantiations are the kernels they were before the flag (DESIGN.md 3.10 states the comparison).
//
// Slots form (awq_sample_tokens_slots, the SLOTS template flag; pinned by tests/test_spec_sampling_cpu.py and
// tests/test_gpu_spec_sampling_kernels.py): the sampler of a speculative verify step.  The launch has B * T logits rows; row
// r = b * T + j is slot j of request b (grid = chunks x T x B, so a block reads b and j from its block index).  Slot (b, j) answers
// "which token would the rows form emit for request b at token index cnt[b] + 1 + j, given the drafts tok[b, 1 .. j] before it":
// it reads params[b] and (PROC) proc[b], the Philox counter is (cnt[b] + 1 + j, b, i / 4, 0), EOS ids are suppressed while
// cnt[b] + 1 + j <= min_new_tokens[b], and the penalty covers history row b OR the bits of tok[b, 1 .. j] (process8 compares the
// <= 7 draft ids, block-uniform loads, with the 8 indices of the thread: no second bitmap; ids outside [0, V) match nothing).
// It writes pred[r] and the status bit r and NOTHING else: cnt, history, tok and finished are read only, there is no ring, no
// latch and no launch-wide step (awq_spec_accept owns them).  A slot of a finished request emits pad and sets no bit.  Every pass
// and combine is the one above on the same arithmetic, so slot (b, j) equals row b of the rows form at that token index and
// history bit for bit (contract E1).  The SLOTS = false instantiations are the kernels they were before the flag.
#include "awq_device.h"
#include "awq_internal.h"

#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr int kChunk = kThreads * kPerThread;
constexpr int kMaxRows = 1024;
constexpr int64_t kMaxVocab = 1 << 20;
constexpr float kFix = 8796093022208.f;  // 2^43: a mass in (0, 1] times this, summed over <= 2^20 tokens, fits a u64
constexpr uint32_t kNone = 0xFFFFFFFFu;

enum : uint32_t { MODE_PAD = 0, MODE_LIVE = 1 };

struct RowState {   // written by one combine, read by the next pass; zeroed by the last combine of the call
    uint32_t mode, maxkey, bin_k, tau_k;
    uint32_t bin_p, need_k, pad0, pad1;
    unsigned long long k_above, z, mass_above, pad2;
};

struct RowWs {      // zero between calls
    unsigned long long best;     // pass 1: key << 32 | ~index
    uint32_t bad, arrive;        // pass 1 NaN / +inf flag; per-row block arrivals (every pass)
    uint32_t cnt_hi[256];        // pass 1
    unsigned long long mass_hi[256];  // pass 2
    uint32_t cnt_lo[256];        // pass 2
    unsigned long long mass_lo[256];  // pass 2
    unsigned long long mass_p[256];   // pass 3
    unsigned long long best_p[256];   // pass 3: score key << 32 | ~index
    unsigned long long best_above;    // pass 3
    unsigned long long pad;
    RowState st;
};

struct WsHead {
    uint32_t arrive;  // rows finished in this launch
    uint32_t pad[63];
};

constexpr size_t kRowBytes = (sizeof(RowWs) + 255) / 256 * 256;
constexpr size_t kHeadBytes = sizeof(WsHead);
static_assert(kHeadBytes % 256 == 0, "head keeps the rows 256-byte aligned");

struct Ctx {
    const uint16_t* logits;
    int64_t row_stride;
    int V;
    int B;
    const AwqSampleParams* params;
    int32_t* t;
    int64_t* out;
    int64_t out_stride;
    int32_t* ring;
    int64_t ring_cap;
    int32_t* finished;
    uint32_t* status;
    char* ws;
};

// The processors' arguments (PROC = true).  A separate type, so that the PROC = false kernels keep Ctx and their argument layout.
struct ProcCtx : Ctx {
    const AwqSampleProc* proc;
    uint32_t* history;
    int64_t history_stride;
};
// The rows form (ROWS = true): params, t and proc point at [B] arrays; types of their own, so that the ROWS = false kernels keep
// their argument layouts.
struct RowsCtx : Ctx {
    const int32_t* max_new;
};
struct RowsProcCtx : ProcCtx {
    const int32_t* max_new;
};
// The slots form (SLOTS = true): params and proc point at [B] arrays, cnt [B] and tok [B, T] replace t, Ctx::B is the launch's
// B * T rows, Ctx::t is not used; types of their own, so that the SLOTS = false kernels keep their argument layouts.
struct SlotsCtx : Ctx {
    const int32_t* cnt;
    const int64_t* tok;
};
struct SlotsProcCtx : ProcCtx {
    const int32_t* cnt;
    const int64_t* tok;
};
template <bool PROC, bool ROWS = false, bool SLOTS = false>
using CtxT = typename std::conditional<
    SLOTS, typename std::conditional<PROC, SlotsProcCtx, SlotsCtx>::type,
    typename std::conditional<ROWS, typename std::conditional<PROC, RowsProcCtx, RowsCtx>::type,
                              typename std::conditional<PROC, ProcCtx, Ctx>::type>::type>::type;

// The parameters, token index and processors of a row: element `row` in the rows form, the one shared struct / word otherwise.
// (An index that folds to 0 in the front end: accessor functions returning references changed the schedule of the ROWS = false pass 3.)
#define AWQ_ROW_OF(ROWS, row) ((ROWS) ? (row) : 0)

// What a block works on.  row: the launch row (logits, workspace, out, status bit).  par: the element of params / proc / t it
// reads.  own: the request's row of finished / history, and the row word of its Philox counter.  slot: its slot in the request.
// Outside the slots form row == own and slot == 0; in the slots form (grid chunks x T x B) row = b * T + j, par = own = b, slot = j.
struct RowId {
    int row, par, own, slot;
};
template <bool ROWS, bool SLOTS> AWQ_DEV RowId row_id() {
    if constexpr (SLOTS) {
        const int b = blockIdx.z, j = blockIdx.y;
        return RowId{b * (int)gridDim.y + j, b, b, j};
    } else {
        const int row = blockIdx.y;
        return RowId{row, AWQ_ROW_OF(ROWS, row), row, 0};
    }
}

AWQ_DEV WsHead* head_of(const Ctx& c) { return reinterpret_cast<WsHead*>(c.ws); }
AWQ_DEV RowWs* row_of(const Ctx& c, int r) { return reinterpret_cast<RowWs*>(c.ws + kHeadBytes + (size_t)r * kRowBytes); }

// ---- agent-scope accesses of every word another block reads in the same launch
template <typename T> AWQ_DEV T ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> AWQ_DEV void st(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> AWQ_DEV void add(T* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
AWQ_DEV void amax(unsigned long long* p, unsigned long long v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the 1-based index of the token the block selects, read at block start: the t word, or in the slots form cnt[b] + 1 + j
template <bool ROWS, bool SLOTS, typename C> AWQ_DEV int32_t token_index(const C& c, const RowId& id) {
    if constexpr (SLOTS)
        return ld(c.cnt + id.par) + 1 + id.slot;
    else
        return ld(c.t + id.par);
}

// fp16 bits -> monotone key (larger key = larger value; -0 == +0)
AWQ_DEV uint32_t key16(uint32_t b) {
    if (b == 0x8000u) b = 0;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
AWQ_DEV float key_to_float(uint32_t k) {
    const uint32_t b = (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu);
    return (float)__builtin_bit_cast(half_t, (uint16_t)b);
}
AWQ_DEV uint32_t fkey32(float f) {  // monotone key of a (non-NaN) fp32 value
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
constexpr uint32_t kFiniteLo = 0x0400u;  // key of -65504; -inf is 0x03FF, NaN below it

AWQ_DEV unsigned long long shfl_xor64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}
AWQ_DEV unsigned long long shfl_up64(unsigned long long v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    return ((unsigned long long)hi << 32) | lo;
}
AWQ_DEV unsigned long long shfl64(unsigned long long v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}
AWQ_DEV unsigned long long wave_max64(unsigned long long v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = shfl_xor64(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// Philox4x64-10, Random123's round and key schedule (numpy's np.random.Philox)
AWQ_DEV void philox4x64_10(unsigned long long c[4], unsigned long long k0, unsigned long long k1) {
    const unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    const unsigned long long W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += W0;
            k1 += W1;
        }
        const unsigned long long hi0 = __umul64hi(M0, c[0]), lo0 = M0 * c[0];
        const unsigned long long hi1 = __umul64hi(M1, c[2]), lo1 = M1 * c[2];
        const unsigned long long n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
    }
}
// exp((l - max) / T) in 2^-43 units: the same expression in passes 2 and 3, so their per-bin sums agree bit for bit
AWQ_DEV unsigned long long mass_fx(float l, float mx, float T) { return (unsigned long long)(expf((l - mx) / T) * kFix + 0.5f); }
// u = ((w >> 41) + 0.5) * 2^-23: exact in fp32 (24 significant bits), so u lies in [2^-24, 1 - 2^-24] and g is finite.
// (With 24 bits, ((w >> 40) + 0.5) rounds to 2^24 for the largest word: u = 1 and g = +inf, a token that wins whatever its logit.)
AWQ_DEV float gumbel(unsigned long long w) {
    const float u = ((float)(uint32_t)(w >> 41) + 0.5f) * 1.1920928955078125e-7f;  // 2^-23
    return -logf(-logf(u));
}

// The 8 logits of this thread (indices i0 .. i0 + 7 of the chunk); h = 0xFC00 (-inf: never counted) past the row end.
AWQ_DEV void load8(const Ctx& c, int row, int i0, uint32_t h[8]) {
    const uint16_t* p = c.logits + (int64_t)row * c.row_stride + i0;
    if (i0 + 8 <= c.V && ((uintptr_t)p & 15u) == 0) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[2 * j] = v[j] & 0xFFFFu;
            h[2 * j + 1] = v[j] >> 16;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = i0 + j < c.V ? (uint32_t)p[j] : 0xFC00u;
    }
}

// The processors (PROC) on the 8 logits of this thread.  eos_on: t <= min_new_tokens (block-uniform).  The history bits of
// i0 .. i0 + 7 are one byte (i0 % 8 == 0): bit v % 8 of byte v / 8 is bit v % 32 of word v / 32 (little endian).
// SLOTS: the history row is the request's, and the drafts in front of the slot, tok[b, 1 .. j], count as seen.
template <bool ROWS, bool SLOTS>
AWQ_DEV void process8(const CtxT<true, ROWS, SLOTS>& c, const AwqSampleParams& P, const RowId& id, int i0, bool eos_on,
                      uint32_t h[8]) {
    if (eos_on) {
        const int n = P.n_eos < 8 ? P.n_eos : 8;
        for (int e = 0; e < n; ++e) {
            const int d = P.eos[e] - i0;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (d == j) h[j] = 0xFC00u;
        }
    }
    const float p = c.proc[id.par].repetition_penalty;
    if (p == 1.f || i0 >= c.V) return;  // (p = 1: v * 1 and v / 1 are v, and fp16(float(h)) is h)
    uint32_t bits = reinterpret_cast<const uint8_t*>(c.history + (int64_t)id.own * c.history_stride)[i0 >> 3];
    if constexpr (SLOTS) {
        const int64_t* in = c.tok + (int64_t)id.own * (int)gridDim.y;
        for (int k = 1; k <= id.slot; ++k) {  // (at most 7, block-uniform)
            const int64_t d = in[k];
            if (d >= i0 && d < i0 + 8 && d < c.V) bits |= 1u << (int)(d - i0);
        }
    }
    if (!bits) return;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (!((bits >> j) & 1u) || (h[j] & 0x7FFFu) >= 0x7C00u) continue;
        float v = (float)__builtin_bit_cast(half_t, (uint16_t)h[j]);
        v = v < 0.f ? v * p : v / p;
        v = fminf(fmaxf(v, -65504.f), 65504.f);
        h[j] = __builtin_bit_cast(uint16_t, (half_t)v);
    }
}

// t <= min_new_tokens, read at block start
template <bool ROWS, bool SLOTS> AWQ_DEV bool eos_suppressed(const CtxT<true, ROWS, SLOTS>& c, const RowId& id) {
    return token_index<ROWS, SLOTS>(c, id) <= c.proc[id.par].min_new_tokens;
}

AWQ_DEV bool is_greedy(const AwqSampleParams& P, int forced) { return forced || P.do_sample == 0 || !(P.temperature > 0.f); }

// The block's arrival on the row counter: true in the last block of the row, after an acquire (the other blocks' atomics are
// visible).  Every thread of every block calls it.  The hand-off recipe of cdna_hip_programming.md G16: every wave drains its
// own atomics, a barrier, ONE lane releases and adds; the last arriver (told by the value its add returned) acquires once,
// drains, and the barrier lets the other waves load.
AWQ_DEV bool arrive_last(RowWs* w) {
    __shared__ uint32_t s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool last = __hip_atomic_fetch_add(&w->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            st(&w->arrive, 0u);
        }
        s_last = last;
    }
    __syncthreads();
    return s_last != 0;
}

AWQ_DEV void set_status(const Ctx& c, int row) {
    __hip_atomic_fetch_or(c.status + (row >> 5), 1u << (row & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Bookkeeping of a finished row (thread 0 of the row's last block); the launch's last row advances t.  sampled: tok was chosen
// from the logits (not the pad of a finished or failed row) -- only then can it latch `finished`.  Nothing written here is
// read by another block of this launch (the next launch reads it), so the launch counter needs no fence; t is read, and
// its load drained, before this row's add, and only the last add's row writes t.
// ROWS: t is the row's own word t[row]; every block of the row has read it before arriving on the row counter, so this block (the
// row's last) advances it here, and the launch counter is not used.  max_new: the row's budget latch.
// SLOTS: the slot's token goes to out[row] and that is all -- no t, ring, finished or history word moves (awq_spec_accept's).
template <bool PROC, bool ROWS, bool SLOTS>
AWQ_DEV void finish_row(const CtxT<PROC, ROWS, SLOTS>& c, int row, const AwqSampleParams& P, int64_t tok, bool sampled) {
    RowWs* w = row_of(c, row);
    const RowState zero{};
    w->st = zero;
    if constexpr (SLOTS) {
        c.out[row] = tok;
        return;
    }
    const int32_t t = ld(c.t + AWQ_ROW_OF(ROWS, row));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    c.out[row * c.out_stride] = tok;
    if (c.ring && t >= 1 && t <= c.ring_cap) c.ring[row * c.ring_cap + (t - 1)] = (int32_t)tok;
    if (c.finished && sampled) {
        const int n = P.n_eos < 8 ? P.n_eos : 8;
        for (int e = 0; e < n; ++e)
            if (tok == P.eos[e]) c.finished[row] = 1;
    }
    if constexpr (PROC) {  // every block of the row has read its history (they all arrived before this combine)
        if (tok >= 0 && tok < c.V)
            __hip_atomic_fetch_or(c.history + row * c.history_stride + (tok >> 5), 1u << (tok & 31), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (ROWS) {
        if (c.finished && c.max_new) {
            const int32_t m = c.max_new[row];
            if (m > 0 && t >= m) c.finished[row] = 1;
        }
        st(c.t + row, t + 1);
    } else {
        WsHead* h = head_of(c);
        if (__hip_atomic_fetch_add(&h->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)c.B - 1) {
            st(&h->arrive, 0u);
            st(c.t, t + 1);
        }
    }
}

// Wave 0 of a combine: the highest bin b (scanning 255 .. 0) whose suffix sum base + sum(v[b..255]) satisfies ok; *above =
// base + sum(v[b+1..255]).  kNone if no bin does.  v[b] is supplied by get(b); every lane of wave 0 calls it.
template <typename Get, typename Ok>
AWQ_DEV uint32_t find_from_top(Get get, unsigned long long base, Ok ok, unsigned long long* above) {
    const int lane = threadIdx.x & 63;
    const int b0 = 255 - 4 * lane;
    unsigned long long v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = get(b0 - j);
        s += v[j];
    }
    unsigned long long incl = s;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = shfl_up64(incl, d);
        if (lane >= d) incl += o;
    }
    const unsigned long long hit = __ballot(ok(base + incl));
    if (!hit) return kNone;
    const int f = __ffsll((long long)hit) - 1;
    uint32_t bin = kNone;
    unsigned long long ab = 0;
    if (lane == f) {
        unsigned long long cum = base + incl - s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (bin == kNone && ok(cum + v[j])) {
                bin = b0 - j;
                ab = cum;
            }
            cum += v[j];
        }
    }
    *above = shfl64(ab, f);
    return (uint32_t)__shfl((int)bin, f, 64);
}

// ---- pass 1 ----------------------------------------------------------------------------------------------------------
template <bool PROC, bool ROWS, bool SLOTS>
__global__ __launch_bounds__(kThreads) void sample_pass1(CtxT<PROC, ROWS, SLOTS> c, int greedy_forced) {
    const RowId id = row_id<ROWS, SLOTS>();
    const int row = id.row, tid = threadIdx.x;
    const AwqSampleParams& P = c.params[id.par];  // (a by-value copy is promoted to 16 KB of LDS / spilled to scratch)
    const bool greedy = is_greedy(P, greedy_forced);
    bool eos_on = false;
    if constexpr (PROC) eos_on = eos_suppressed<ROWS, SLOTS>(c, id);
    RowWs* w = row_of(c, row);
    const bool fin = c.finished && c.finished[id.own] != 0;
    __shared__ uint32_t s_cnt[256];
    __shared__ unsigned long long s_best[kThreads / 64];
    __shared__ uint32_t s_bad;
    s_cnt[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (!fin) {
        const int i0 = blockIdx.x * kChunk + tid * kPerThread;
        uint32_t h[8];
        load8(c, row, i0, h);
        if constexpr (PROC) process8<ROWS, SLOTS>(c, P, id, i0, eos_on, h);
        unsigned long long best = 0;
        uint32_t bad = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if ((h[j] & 0x7FFFu) >= 0x7C00u) {  // inf / NaN: -inf is skipped, the rest poisons the row
                bad |= h[j] != 0xFC00u;
                continue;
            }
            const uint32_t k = key16(h[j]);
            const unsigned long long packed = ((unsigned long long)k << 32) | (0xFFFFFFFFu - (uint32_t)(i0 + j));
            best = packed > best ? packed : best;
            if (!greedy) atomicAdd(&s_cnt[k >> 8], 1u);
        }
        best = wave_max64(best);
        if (__any(bad) && (tid & 63) == 0) s_bad = 1;
        if ((tid & 63) == 0) s_best[tid >> 6] = best;
    }
    __syncthreads();
    if (!fin) {
        if (tid == 0) {
            unsigned long long b = 0;
            for (int q = 0; q < kThreads / 64; ++q) b = s_best[q] > b ? s_best[q] : b;
            if (b) amax(&w->best, b);
            if (s_bad) st(&w->bad, 1u);
        }
        if (!greedy && s_cnt[tid]) add(&w->cnt_hi[tid], s_cnt[tid]);
    }
    if (!arrive_last(w)) return;

    // ---- combine (the row's last block)
    const unsigned long long best = ld(&w->best);
    const uint32_t bad = ld(&w->bad);
    uint32_t cnt = 0;
    if (!greedy) {
        cnt = ld(&w->cnt_hi[tid]);
        st(&w->cnt_hi[tid], 0u);
    }
    __syncthreads();
    if (tid == 0) {
        st(&w->best, 0ull);
        st(&w->bad, 0u);
    }
    const uint32_t maxkey = (uint32_t)(best >> 32);
    const bool live = !fin && !bad && best != 0;
    if (!fin && !live && tid == 0) set_status(c, row);
    if (greedy) {
        if (tid == 0) finish_row<PROC, ROWS, SLOTS>(c, row, P, live ? (int64_t)(0xFFFFFFFFu - (uint32_t)best) : (int64_t)P.pad, live);
        return;
    }
    __shared__ uint32_t s_hist[256];
    s_hist[tid] = cnt;
    __syncthreads();
    if (tid >= 64) return;
    // top-k boundary bin: active when 0 < k < number of finite tokens
    uint32_t bin_k = kNone;
    unsigned long long k_above = 0;
    if (live && P.top_k > 0) {
        const unsigned long long k = (unsigned long long)P.top_k;
        bin_k = find_from_top([&](int b) { return (unsigned long long)s_hist[b]; }, 0ull,
                              [&](unsigned long long cum) { return cum >= k; }, &k_above);
    }
    if (tid == 0) {
        RowState s{};
        s.mode = live ? MODE_LIVE : MODE_PAD;
        s.maxkey = maxkey;
        s.need_k = bin_k != kNone;
        s.bin_k = bin_k != kNone ? bin_k : (kFiniteLo >> 8);
        s.tau_k = kFiniteLo;
        s.k_above = k_above;
        w->st = s;
    }
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------
template <bool PROC, bool ROWS, bool SLOTS>
__global__ __launch_bounds__(kThreads) void sample_pass2(CtxT<PROC, ROWS, SLOTS> c, int greedy_forced) {
    const RowId id = row_id<ROWS, SLOTS>();
    const int row = id.row, tid = threadIdx.x;
    const AwqSampleParams& P = c.params[id.par];  // (a by-value copy is promoted to 16 KB of LDS / spilled to scratch)
    if (is_greedy(P, greedy_forced)) return;
    bool eos_on = false;
    if constexpr (PROC) eos_on = eos_suppressed<ROWS, SLOTS>(c, id);
    RowWs* w = row_of(c, row);
    const RowState S = w->st;
    const bool topp = P.top_p < 1.f;
    const bool work = S.mode == MODE_LIVE && (S.need_k || topp);
    __shared__ unsigned long long s_mhi[256], s_mlo[256];
    __shared__ uint32_t s_clo[256];
    s_mhi[tid] = 0;
    s_mlo[tid] = 0;
    s_clo[tid] = 0;
    __syncthreads();
    if (work) {
        const float mx = key_to_float(S.maxkey), T = P.temperature;
        const int i0 = blockIdx.x * kChunk + tid * kPerThread;
        uint32_t h[8];
        load8(c, row, i0, h);
        if constexpr (PROC) process8<ROWS, SLOTS>(c, P, id, i0, eos_on, h);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if ((h[j] & 0x7FFFu) >= 0x7C00u) continue;
            const uint32_t k = key16(h[j]), hi = k >> 8;
            if (hi < S.bin_k) continue;
            const unsigned long long m =
                topp ? mass_fx((float)__builtin_bit_cast(half_t, (uint16_t)h[j]), mx, T) : 0ull;
            if (hi > S.bin_k) {
                if (m) atomicAdd(&s_mhi[hi], m);
            } else {
                atomicAdd(&s_clo[k & 0xFFu], 1u);
                if (m) atomicAdd(&s_mlo[k & 0xFFu], m);
            }
        }
        __syncthreads();
        if (s_mhi[tid]) add(&w->mass_hi[tid], s_mhi[tid]);
        if (s_mlo[tid]) add(&w->mass_lo[tid], s_mlo[tid]);
        if (s_clo[tid]) add(&w->cnt_lo[tid], s_clo[tid]);
    }
    if (!arrive_last(w)) return;

    __syncthreads();
    s_mhi[tid] = ld(&w->mass_hi[tid]);
    s_mlo[tid] = ld(&w->mass_lo[tid]);
    s_clo[tid] = ld(&w->cnt_lo[tid]);
    st(&w->mass_hi[tid], 0ull);
    st(&w->mass_lo[tid], 0ull);
    st(&w->cnt_lo[tid], 0u);
    __syncthreads();
    if (tid >= 64 || S.mode != MODE_LIVE) return;
    RowState s = S;
    uint32_t lo_k = 0;
    if (S.need_k) {  // the top-k threshold inside its bin
        unsigned long long dummy;
        const unsigned long long k = (unsigned long long)P.top_k;
        lo_k = find_from_top([&](int b) { return (unsigned long long)s_clo[b]; }, S.k_above,
                             [&](unsigned long long cum) { return cum >= k; }, &dummy);
        if (lo_k == kNone) lo_k = 0;  // (cannot happen: pass 1 counted the same tokens)
        s.tau_k = (S.bin_k << 8) | lo_k;
    }
    s.bin_p = kNone;
    if (topp) {  // kept mass Z, then the top-p boundary bin
        const uint32_t bk = S.bin_k;
        const int lane = tid;
        // Z: the bins above the top-k bin whole, the top-k bin from its low-byte masses at or above the threshold
        unsigned long long zk = 0, part = 0;
        for (int l = lane; l < 256; l += 64) {
            zk += l >= (int)lo_k ? s_mlo[l] : 0ull;
            part += l > (int)bk ? s_mhi[l] : 0ull;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            zk += shfl_xor64(zk, m);
            part += shfl_xor64(part, m);
        }
        const unsigned long long Z = part + zk;
        const double target = (double)P.top_p * (double)Z;
        unsigned long long above = 0;
        const uint32_t bp = find_from_top([&](int b) { return b > (int)bk ? s_mhi[b] : b == (int)bk ? zk : 0ull; }, 0ull,
                                          [&](unsigned long long cum) { return (double)cum >= target; }, &above);
        s.z = Z;
        s.bin_p = bp != kNone ? bp : bk;  // (cannot miss: the suffix at bin_k is Z)
        s.mass_above = bp != kNone ? above : 0ull;
    }
    if (tid == 0) w->st = s;
}

// ---- pass 3 ----------------------------------------------------------------------------------------------------------
template <bool PROC, bool ROWS, bool SLOTS>
__global__ __launch_bounds__(kThreads) void sample_pass3(CtxT<PROC, ROWS, SLOTS> c, int greedy_forced) {
    const RowId id = row_id<ROWS, SLOTS>();
    const int row = id.row, tid = threadIdx.x;
    const AwqSampleParams& P = c.params[id.par];  // (a by-value copy is promoted to 16 KB of LDS / spilled to scratch)
    if (is_greedy(P, greedy_forced)) return;
    bool eos_on = false;
    if constexpr (PROC) eos_on = eos_suppressed<ROWS, SLOTS>(c, id);
    RowWs* w = row_of(c, row);
    const RowState S = w->st;
    const bool topp = S.bin_p != kNone && P.top_p < 1.f;
    __shared__ unsigned long long s_m[256], s_b[256], s_best[kThreads / 64];
    s_m[tid] = 0;
    s_b[tid] = 0;
    __syncthreads();
    if (S.mode == MODE_LIVE) {
        const float mx = key_to_float(S.maxkey), T = P.temperature;
        const unsigned long long seed = P.seed, t = (unsigned long long)token_index<ROWS, SLOTS>(c, id);
        const int i0 = blockIdx.x * kChunk + tid * kPerThread;
        uint32_t h[8];
        load8(c, row, i0, h);
        if constexpr (PROC) process8<ROWS, SLOTS>(c, P, id, i0, eos_on, h);
        const uint32_t lo_key = topp ? (S.bin_p << 8) : S.tau_k;
        const uint32_t tau = lo_key > S.tau_k ? lo_key : S.tau_k;
        unsigned long long best = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            bool any = false;
            uint32_t kk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t b = h[4 * q + j];
                kk[j] = ((b & 0x7FFFu) >= 0x7C00u) ? 0u : key16(b);
                any |= kk[j] >= tau;
            }
            if (!any) continue;
            unsigned long long ctr[4] = {t, (unsigned long long)id.own, (unsigned long long)((i0 >> 2) + q), 0ull};
            philox4x64_10(ctr, seed, 0ull);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (kk[j] < tau) continue;
                const float l = (float)__builtin_bit_cast(half_t, (uint16_t)h[4 * q + j]);
                const float score = l / T + gumbel(ctr[j]);
                const uint32_t idx = (uint32_t)(i0 + 4 * q + j);
                const unsigned long long packed = ((unsigned long long)fkey32(score) << 32) | (0xFFFFFFFFu - idx);
                if (topp && (kk[j] >> 8) == S.bin_p) {
                    const unsigned long long m = mass_fx(l, mx, T);
                    if (m) atomicAdd(&s_m[kk[j] & 0xFFu], m);
                    atomicMax(&s_b[kk[j] & 0xFFu], packed);
                } else {
                    best = packed > best ? packed : best;
                }
            }
        }
        best = wave_max64(best);
        if ((tid & 63) == 0) s_best[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long b = 0;
            for (int x = 0; x < kThreads / 64; ++x) b = s_best[x] > b ? s_best[x] : b;
            if (b) amax(&w->best_above, b);
        }
        if (s_m[tid]) add(&w->mass_p[tid], s_m[tid]);
        if (s_b[tid]) amax(&w->best_p[tid], s_b[tid]);
    }
    if (!arrive_last(w)) return;

    __syncthreads();
    s_m[tid] = ld(&w->mass_p[tid]);
    s_b[tid] = ld(&w->best_p[tid]);
    st(&w->mass_p[tid], 0ull);
    st(&w->best_p[tid], 0ull);
    const unsigned long long above_best = ld(&w->best_above);
    __syncthreads();
    if (tid == 0) st(&w->best_above, 0ull);
    if (tid >= 64) return;
    if (S.mode != MODE_LIVE) {
        if (tid == 0) finish_row<PROC, ROWS, SLOTS>(c, row, P, (int64_t)P.pad, false);
        return;
    }
    uint32_t lo_p = 0;
    if (topp) {
        const double target = (double)P.top_p * (double)S.z;
        unsigned long long dummy;
        lo_p = find_from_top([&](int b) { return s_m[b]; }, S.mass_above,
                             [&](unsigned long long cum) { return (double)cum >= target; }, &dummy);
        if (lo_p == kNone) lo_p = 0;
    }
    unsigned long long best = 0;
    for (int l = tid; l < 256; l += 64)
        if ((uint32_t)l >= lo_p && s_b[l] > best) best = s_b[l];
    best = wave_max64(best);
    best = above_best > best ? above_best : best;
    if (tid == 0) {
        if (!best) set_status(c, row);
        finish_row<PROC, ROWS, SLOTS>(c, row, P, best ? (int64_t)(0xFFFFFFFFu - (uint32_t)best) : (int64_t)P.pad, best != 0);
    }
}

}  // namespace

size_t awq_sample_workspace_bytes(int64_t B, int64_t V) {
    if (B < 1 || B > kMaxRows || V < 1 || V > kMaxVocab) return 0;
    return kHeadBytes + (size_t)B * kRowBytes;
}

namespace {

// validation of the launch arguments shared by awq_sample_tokens, awq_sample_tokens_ex and awq_sample_tokens_rows (A: AwqSampleArgs
// or AwqSampleRowsArgs, which carries the same fields); AWQ_OK and *c filled, or the error
template <typename A>
int sample_ctx(const A* a, Ctx* c) {
    if (!a) return AWQ_ERR_NULL;
    if (a->struct_bytes != sizeof(A)) return AWQ_ERR_BAD_SHAPE;
    if (a->B < 1 || a->B > kMaxRows || a->V < 1 || a->V > kMaxVocab) return AWQ_ERR_UNSUPPORTED;
    if (a->row_stride < a->V && a->B > 1) return AWQ_ERR_BAD_SHAPE;
    if (!a->logits || !a->params || !a->t || !a->out || !a->status || !a->workspace) return AWQ_ERR_NULL;
    if (a->ring && a->ring_cap < 1) return AWQ_ERR_BAD_SHAPE;
    if (a->workspace_bytes < awq_sample_workspace_bytes(a->B, a->V)) return AWQ_ERR_WORKSPACE;
    if (((uintptr_t)a->workspace & 255u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    if (((uintptr_t)a->logits & 1u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    *c = Ctx{};
    c->logits = a->logits;
    c->row_stride = a->row_stride;
    c->V = (int)a->V;
    c->B = (int)a->B;
    c->params = a->params;
    c->t = a->t;
    c->out = a->out;
    c->out_stride = a->out_stride;
    c->ring = a->ring;
    c->ring_cap = a->ring_cap;
    c->finished = a->finished;
    c->status = a->status;
    c->ws = static_cast<char*>(a->workspace);
    return AWQ_OK;
}

// grid: chunks x rows; the slots form (a->T: AwqSampleSlotsArgs) chunks x T x B
template <bool PROC, bool ROWS = false, bool SLOTS = false, typename A>
int sample_run(const A* a, const CtxT<PROC, ROWS, SLOTS>& c) {
    const hipStream_t s = static_cast<hipStream_t>(a->stream);
    const int greedy = (a->flags & AWQ_SAMPLE_FLAG_GREEDY) != 0;
    dim3 grid((unsigned)((a->V + kChunk - 1) / kChunk), (unsigned)a->B);
    if constexpr (SLOTS) grid = dim3(grid.x, (unsigned)a->T, (unsigned)a->B);
    hipLaunchKernelGGL((sample_pass1<PROC, ROWS, SLOTS>), grid, dim3(kThreads), 0, s, c, greedy);
    if (!greedy) {
        hipLaunchKernelGGL((sample_pass2<PROC, ROWS, SLOTS>), grid, dim3(kThreads), 0, s, c, 0);
        hipLaunchKernelGGL((sample_pass3<PROC, ROWS, SLOTS>), grid, dim3(kThreads), 0, s, c, 0);
    }
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

// one thread per id: ORs bit ids[b, s] of history row b (ids outside [0, V) ignored)
__global__ __launch_bounds__(kThreads) void sample_history_seed_kernel(uint32_t* history, int64_t history_stride,
                                                                       const int64_t* ids, int64_t ids_stride, int64_t S,
                                                                       int64_t V) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (s >= S) return;
    const int64_t v = ids[b * ids_stride + s];
    if (v < 0 || v >= V) return;
    __hip_atomic_fetch_or(history + b * history_stride + (v >> 5), 1u << (v & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

int awq_sample_tokens(const AwqSampleArgs* a) {
    Ctx c;
    const int rc = sample_ctx(a, &c);
    return rc != AWQ_OK ? rc : sample_run<false>(a, c);
}

int awq_sample_tokens_ex(const AwqSampleArgs* a, const AwqSampleProcArgs* q) {
    if (!q) return awq_sample_tokens(a);
    ProcCtx c;
    const int rc = sample_ctx(a, &c);
    if (rc != AWQ_OK) return rc;
    if (q->struct_bytes != sizeof(AwqSampleProcArgs)) return AWQ_ERR_BAD_SHAPE;
    if (q->flags != 0) return AWQ_ERR_UNSUPPORTED;
    if (!q->proc || !q->history) return AWQ_ERR_NULL;
    if (q->history_stride < (a->V + 31) / 32) return AWQ_ERR_BAD_SHAPE;
    if (((uintptr_t)q->history & 3u) != 0 || ((uintptr_t)q->proc & 15u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    c.proc = q->proc;
    c.history = q->history;
    c.history_stride = q->history_stride;
    return sample_run<true>(a, c);
}

int awq_sample_tokens_rows(const AwqSampleRowsArgs* a) {
    RowsProcCtx c;
    const int rc = sample_ctx(a, &c);
    if (rc != AWQ_OK) return rc;
    if (((uintptr_t)a->params & 7u) != 0 || ((uintptr_t)a->t & 3u) != 0 || ((uintptr_t)a->max_new & 3u) != 0)
        return AWQ_ERR_BAD_ALIGNMENT;
    if (a->max_new && !a->finished) return AWQ_ERR_NULL;  // the budget latch is a finished flag
    c.max_new = a->max_new;
    if (!a->proc && !a->history) {
        RowsCtx r;
        static_cast<Ctx&>(r) = c;
        r.max_new = a->max_new;
        return sample_run<false, true>(a, r);
    }
    if (!a->proc || !a->history) return AWQ_ERR_NULL;  // they go together
    if (a->history_stride < (a->V + 31) / 32) return AWQ_ERR_BAD_SHAPE;
    if (((uintptr_t)a->history & 3u) != 0 || ((uintptr_t)a->proc & 15u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    c.proc = a->proc;
    c.history = a->history;
    c.history_stride = a->history_stride;
    return sample_run<true, true>(a, c);
}

int awq_sample_tokens_slots(const AwqSampleSlotsArgs* a) {
    if (!a) return AWQ_ERR_NULL;
    if (a->struct_bytes != sizeof(AwqSampleSlotsArgs)) return AWQ_ERR_BAD_SHAPE;
    if (a->T < 2 || a->T > 8 || a->B < 1 || a->B * a->T > kMaxRows || a->V < 1 || a->V > kMaxVocab) return AWQ_ERR_UNSUPPORTED;
    const int64_t rows = a->B * a->T;
    if (a->row_stride < a->V) return AWQ_ERR_BAD_SHAPE;  // (rows >= 2)
    if (!a->logits || !a->params || !a->cnt || !a->tok || !a->pred || !a->status || !a->workspace) return AWQ_ERR_NULL;
    if (a->workspace_bytes < awq_sample_workspace_bytes(rows, a->V)) return AWQ_ERR_WORKSPACE;
    if (((uintptr_t)a->workspace & 255u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    if (((uintptr_t)a->logits & 1u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    if (((uintptr_t)a->params & 7u) != 0 || ((uintptr_t)a->cnt & 3u) != 0 || ((uintptr_t)a->tok & 7u) != 0 ||
        ((uintptr_t)a->pred & 7u) != 0 || ((uintptr_t)a->finished & 3u) != 0 || ((uintptr_t)a->status & 3u) != 0)
        return AWQ_ERR_BAD_ALIGNMENT;
    SlotsProcCtx c{};
    c.logits = a->logits;
    c.row_stride = a->row_stride;
    c.V = (int)a->V;
    c.B = (int)rows;
    c.params = a->params;
    c.out = a->pred;
    c.out_stride = 1;
    c.finished = const_cast<int32_t*>(a->finished);  // (read only: the slots kernels never latch)
    c.status = a->status;
    c.ws = static_cast<char*>(a->workspace);
    c.cnt = a->cnt;
    c.tok = a->tok;
    if (!a->proc && !a->history) {
        SlotsCtx r{};
        static_cast<Ctx&>(r) = c;
        r.cnt = a->cnt;
        r.tok = a->tok;
        return sample_run<false, false, true>(a, r);
    }
    if (!a->proc || !a->history) return AWQ_ERR_NULL;  // they go together
    if (a->history_stride < (a->V + 31) / 32) return AWQ_ERR_BAD_SHAPE;
    if (((uintptr_t)a->history & 3u) != 0 || ((uintptr_t)a->proc & 15u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    c.proc = a->proc;
    c.history = const_cast<uint32_t*>(a->history);    // (read only)
    c.history_stride = a->history_stride;
    return sample_run<true, false, true>(a, c);
}

int awq_sample_history_seed(uint32_t* history, int64_t history_stride, const int64_t* ids, int64_t ids_stride, int64_t B,
                            int64_t S, int64_t V, void* stream) {
    if (B < 0 || B > kMaxRows || S < 0 || S > 0x7FFFFFFF || V < 1 || V > kMaxVocab) return AWQ_ERR_UNSUPPORTED;
    if (B == 0 || S == 0) return AWQ_OK;
    if (!history || !ids) return AWQ_ERR_NULL;
    if (history_stride < (V + 31) / 32 || (B > 1 && ids_stride < S)) return AWQ_ERR_BAD_SHAPE;
    if (((uintptr_t)history & 3u) != 0 || ((uintptr_t)ids & 7u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
    const dim3 grid((unsigned)((S + kThreads - 1) / kThreads), (unsigned)B);
    hipLaunchKernelGGL(sample_history_seed_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), history,
                       history_stride, ids, ids_stride, S, V);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}
