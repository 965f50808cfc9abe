// spec.hip -- the integer half of speculative decoding (awq_spec_accept / awq_spec_accept_ex, awq_ngram_draft; include/awq_hip.h): which of a verify
// step's T tokens a row keeps, and the next step's drafts by prompt lookup.  One block per sequence, no host involvement,
// capturable; every word lives in device memory the decoder owns (modules/fused/decode.py), the parameters in struct
// AwqSpecParams there, so one captured launch serves every call.  tests/spec_ref.py restates both rules in numpy; the kernels
// agree with it exactly.
#include "awq_device.h"
#include "awq_internal.h"

namespace {

struct SpecWords {
    const AwqSpecParams* params;
    int64_t* tok;
    const int64_t* pred;
    int32_t* hist;
    int32_t* n_hist;
    int32_t* cnt;
    int32_t* ring;
    int32_t* finished;
    int32_t* pos_rows;
    int32_t* len_rows;
    const uint32_t* status;
    int32_t* steps;
    int T, hist_cap, ring_cap;
    uint32_t* history;  // awq_spec_accept_ex: the sampler's penalty bitmap [B, history_stride], or NULL
    int64_t history_stride;
    int V;
};

// Acceptance: a handful of words per row -- thread 0 of the row's block walks the T slots.
__global__ __launch_bounds__(64) void awq_spec_accept_kernel(SpecWords w) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x, T = w.T;
    if (w.finished[b]) return;  // a finished row emits nothing and its words do not move
    const AwqSpecParams P = *w.params;
    const int64_t* in = w.tok + (int64_t)b * T;
    const int64_t* pred = w.pred + (int64_t)b * T;
    if (w.status) {  // a slot of this row held NaN / +inf logits: the row ends here (the sticky bit stays for the host)
        bool bad = false;
        for (int j = 0; j < T; ++j) {
            const int row = b * T + j;
            bad |= (w.status[row >> 5] >> (row & 31)) & 1u;
        }
        if (bad) {
            w.finished[b] = 1;
            return;
        }
    }
    int a = 0;
    while (a < T - 1 && in[a + 1] == pred[a]) ++a;
    const int n_eos = max(0, min(P.n_eos, 8));
    int cnt = w.cnt[b], nh = w.n_hist[b];
    const int budget = P.max_new_tokens - cnt;
    int m = 0;
    bool done = budget <= 0;
    while (!done && m <= a) {
        const int tk = (int)pred[m];
        if (cnt + m < w.ring_cap) w.ring[(int64_t)b * w.ring_cap + cnt + m] = tk;
        if (nh + m >= 0 && nh + m < w.hist_cap) w.hist[(int64_t)b * w.hist_cap + nh + m] = tk;
        if (w.history && tk >= 0 && tk < w.V) w.history[(int64_t)b * w.history_stride + (tk >> 5)] |= 1u << (tk & 31);  // (the row's one writer)
        ++m;
        for (int e = 0; e < n_eos; ++e) done |= tk == P.eos[e];
        done |= m >= budget;
    }
    w.cnt[b] = cnt + m;
    w.n_hist[b] = nh + m;
    w.pos_rows[b] += m;
    w.len_rows[b] += m;
    if (w.steps && m) w.steps[b] += 1;
    if (done) w.finished[b] = 1;
}

// Drafts by prompt lookup.  For every continuation start e in [1, n - 1] (e = s + g) the block counts how many tokens in front of e
// equal the tokens in front of n: k(e) = the largest k <= min(ngram_max, e) with h[e - i] == h[n - i] for i = 1 .. k.  An n-gram of
// length g matches at s = e - g exactly when k(e) >= g, so "the largest s for g" is best[g] = max { e : k(e) >= g }: one coalesced
// block-wide scan of the row (thread x takes e = 1 + x, 1 + x + 256, ...) serves every g at once.
constexpr int SPEC_NGRAM_MAX = 8;
__global__ __launch_bounds__(256) void awq_ngram_draft_kernel(SpecWords w) {
    __shared__ int best[SPEC_NGRAM_MAX + 1];
    const int b = blockIdx.x, T = w.T;
    const int n = min(w.n_hist[b], w.hist_cap);
    if (n < 1) return;
    const int32_t* h = w.hist + (int64_t)b * w.hist_cap;
    const int gmax = max(1, min(w.params->ngram_max, SPEC_NGRAM_MAX));
    if (threadIdx.x <= SPEC_NGRAM_MAX) best[threadIdx.x] = 0;
    __syncthreads();
    int suffix[SPEC_NGRAM_MAX];
#pragma unroll
    for (int i = 0; i < SPEC_NGRAM_MAX; ++i) suffix[i] = (i < gmax && n - 1 - i >= 0) ? h[n - 1 - i] : -1;  // h[n - 1 - i]
    int mine[SPEC_NGRAM_MAX + 1];
#pragma unroll
    for (int g = 0; g <= SPEC_NGRAM_MAX; ++g) mine[g] = 0;
    for (int e = 1 + (int)threadIdx.x; e <= n - 1; e += 256) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < SPEC_NGRAM_MAX; ++i) {
            ok = ok && i < gmax && e - 1 - i >= 0 && h[max(e - 1 - i, 0)] == suffix[i];
            if (ok) mine[i + 1] = e;  // (e grows along the loop: the last one kept is the largest)
        }
    }
#pragma unroll
    for (int g = 1; g <= SPEC_NGRAM_MAX; ++g)
        if (mine[g]) atomicMax(&best[g], mine[g]);
    __syncthreads();
    if (threadIdx.x < T) {
        const int i = (int)threadIdx.x - 1;  // draft slot; -1: slot 0, the row's last token
        int e = 0;
        for (int g = gmax; g >= 1 && !e; --g) e = best[g];
        const int last = h[n - 1];
        int tk = last;
        if (i >= 0 && e && e + i < n) tk = h[e + i];
        w.tok[(int64_t)b * T + threadIdx.x] = tk;
    }
}

int spec_words(const AwqSpecArgs* a, bool accept, SpecWords* w) {
    if (!a || a->struct_bytes != sizeof(AwqSpecArgs)) return AWQ_ERR_BAD_SHAPE;
    if (a->B < 0 || a->B > 65535 || a->hist_cap < 1 || a->hist_cap > INT32_MAX || a->ring_cap < 0 || a->ring_cap > INT32_MAX)
        return AWQ_ERR_BAD_SHAPE;
    if (a->T < 2 || a->T > 8) return AWQ_ERR_UNSUPPORTED;
    if (!a->params || !a->tok || !a->hist || !a->n_hist) return AWQ_ERR_NULL;
    if (accept && (!a->pred || !a->cnt || !a->ring || !a->finished || !a->pos_rows || !a->len_rows)) return AWQ_ERR_NULL;
    *w = SpecWords{a->params, a->tok, a->pred, a->hist, a->n_hist, a->cnt, a->ring, a->finished, a->pos_rows, a->len_rows,
                   a->status, a->steps, (int)a->T, (int)a->hist_cap, (int)a->ring_cap, nullptr, 0, 0};
    return AWQ_OK;
}

}  // namespace

int awq_spec_accept(const AwqSpecArgs* a) { return awq_spec_accept_ex(a, nullptr); }

int awq_spec_accept_ex(const AwqSpecArgs* a, const AwqSpecHistoryArgs* q) {
    SpecWords w;
    if (int rc = spec_words(a, true, &w)) return rc;
    if (q) {
        if (q->struct_bytes != sizeof(AwqSpecHistoryArgs)) return AWQ_ERR_BAD_SHAPE;
        if (q->flags != 0 || q->V < 1 || q->V > (1 << 20)) return AWQ_ERR_UNSUPPORTED;
        if (!q->history) return AWQ_ERR_NULL;
        if (q->history_stride < (q->V + 31) / 32) return AWQ_ERR_BAD_SHAPE;
        if (((uintptr_t)q->history & 3u) != 0) return AWQ_ERR_BAD_ALIGNMENT;
        w.history = q->history;
        w.history_stride = q->history_stride;
        w.V = (int)q->V;
    }
    if (a->B == 0) return AWQ_OK;
    hipLaunchKernelGGL(awq_spec_accept_kernel, dim3((unsigned)a->B), dim3(64), 0, static_cast<hipStream_t>(a->stream), w);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

int awq_ngram_draft(const AwqSpecArgs* a) {
    SpecWords w;
    if (int rc = spec_words(a, false, &w)) return rc;
    if (a->B == 0) return AWQ_OK;
    hipLaunchKernelGGL(awq_ngram_draft_kernel, dim3((unsigned)a->B), dim3(256), 0, static_cast<hipStream_t>(a->stream), w);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}
