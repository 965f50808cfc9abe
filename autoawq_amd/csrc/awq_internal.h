// awq_internal.h -- host-side launcher prototypes shared between the .hip translation units
// and capi.hip.  Not part of the public ABI (that is include/awq_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/awq_hip.h"
#include <atomic>

// The opt-in to more than 64 KB of dynamic LDS is an attribute of a kernel ON A DEVICE: asked for once per (kernel, device)
// -- the call sites keep one bit per device ordinal -- thread-safe, idempotent, no other process-wide state (a
// function-local `static const bool` did it once per PROCESS, i.e. for the first device only).
inline bool awq_lds_opt_in(const void* kernel, std::atomic<unsigned long long>& done, int bytes = 160 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    done.fetch_or(bit, std::memory_order_release);
    return true;
}

int awq_launch_dequant(const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, uint16_t* out,
                       int64_t K, int64_t N, int64_t g, hipStream_t stream);
int awq_launch_unpack(const int32_t* q, uint8_t* out, int64_t rows, int64_t words, hipStream_t stream);

// Division by a run-time constant without an integer divide on the device: (x * magic) >> 32 == x / d for every x < limit.
// magic = floor(2^32 / d) + 1 is exact while x * (magic * d - 2^32) < 2^32.  False if d == 1 or the range is too large.
inline bool awq_magic_u32(uint32_t d, uint32_t limit, uint32_t* out) {
    if (d < 2) return false;
    const uint64_t m = ((uint64_t)1 << 32) / d + 1;
    const uint64_t e = m * d - ((uint64_t)1 << 32);  // 1 .. d
    if ((uint64_t)limit * e >= ((uint64_t)1 << 32)) return false;
    *out = (uint32_t)m;
    return true;
}

struct AwqGemmArgs {
    const uint16_t* x;       // [M, K] fp16
    const int32_t* qweight;  // [K, N/8]
    const uint16_t* scales;  // [K/g, N]
    const int32_t* qzeros;   // [K/g, N/8]
    const uint16_t* bias = nullptr;  // [N] or null
    uint16_t* y;             // [M, N]
    int M, K, N, g;
    int x_gated = 0;  // decode kernel only: 1 = x is [M, 2K] = [gate | up], stage silu(gate) * up; 2 = stage rmsnorm(x + res_in)
    const uint16_t* res_in = nullptr;   // mode 2: optional residual rows [M, K]
    uint16_t* res_out = nullptr;        // mode 2: fp16(x + res_in) is written here (must not alias res_in)
    const uint16_t* norm_w = nullptr;   // mode 2: norm weight [K]
    float norm_eps = 0.f;
    const float* ssq_in = nullptr;      // mode 2: [M, ssq_in_tiles] row sums of squares from the producing call
    int ssq_in_tiles = 0;
    const uint16_t* add_res = nullptr;  // epilogue (decode kernel, M <= 4): y = fp16(fp16(x W + bias) + add_res)
    float* ssq_out = nullptr;           // epilogue: [M, ceil(N / 256)] sums of squares of y per 256-column tile
    // the workspace (none unless capi.hip carves one):
    int* counters = nullptr;    // control words (word 0 = error flag), zero on entry
    float* exchange = nullptr;  // in-launch split-K exchange region: all-ones sentinel on entry AND on exit
    size_t exchange_bytes = 0;
    float* partial = nullptr;   // scratch fp32 slabs for the two-pass reducers (no invariant between calls)
    size_t partial_floats = 0;
    hipStream_t stream;
};

// The routing of a grouped (MoE) launch over stacked expert tensors, beside the AwqGemmArgs of one expert's product.
struct AwqGroupedArgs {
    const float* pair_weights = nullptr;  // [num_pairs] routing weights by pair index, or null
    int x_div = 1;                        // pair i (a gathered row r: row_map[r]) reads activation row i / x_div
    // token blocks (awq_launch_grouped_gemm): block b gathers rows sorted_ids[M b .. M b + M - 1] for expert expert_ids[b]
    const int32_t *sorted_ids = nullptr, *expert_ids = nullptr, *num_post_pad = nullptr;
    int num_pairs = 0, max_blocks = 0;
    int64_t expert_qw_words = 0, expert_z_words = 0, expert_s_halfs = 0;  // strides of the expert stacks
    // rows sorted by expert (awq_launch_gemm_regb_grouped): seg [num_experts + 1] row offsets on the device; row_map / gather /
    // scatter: see RegbParams (all optional; without row_map the rows of x and y are the sorted rows)
    const int32_t *seg = nullptr, *row_map = nullptr;
    int num_experts = 0;
    bool gather = false, scatter = false;
};

int awq_launch_gemm_naive(const AwqGemmArgs& a);
// Reference-order-numerics GEMV (M <= 4).  nlog: log2 of column-lanes per wave (2..4), splitk >= 1.
int awq_launch_gemv_valu(const AwqGemmArgs& a, int nlog, int splitk, bool nt);
int awq_gemv_valu_default_split(int K, int N, int nlog);
int awq_launch_splitk_reduce(const AwqGemmArgs& a, int splitk);
// MFMA decode GEMV / skinny GEMM, M <= 16.  wpl: packed words per lane (2|4); nwaves: waves per
// block (2|4|8); unit: 16-row sets per wave iteration (2|4|8); splitk: K slices.  0 = auto each.
bool awq_gemv_mfma_supports(int M, int K, int N, int g, int wpl);
int awq_launch_gemv_mfma(const AwqGemmArgs& a, int wpl, int nwaves, int unit, int splitk, bool two_pass);
// Fused dequant + LDS-tiled MFMA GEMM, any M (meant for M > 16).  bn: block tile width (128|256, 0 = auto).
bool awq_gemm_tiled_supports(int M, int K, int N, int g);
int awq_launch_gemm_tiled(const AwqGemmArgs& a, int bn, int splitk);
// Prefill GEMM with the weight operand decoded in registers (gemm_regb.hip).  bm: rows per block tile (128|256, 0 = auto).
bool awq_gemm_regb_supports(int M, int K, int N, int g);
int awq_launch_gemm_regb(const AwqGemmArgs& a, int bm);
// Batched-decode GEMM, 17 <= M <= 64, weights decoded in registers, no barrier in the K loop (gemm_skinny.hip).
bool awq_gemm_skinny_supports(int M, int K, int N, int g);
int awq_launch_gemm_skinny(const AwqGemmArgs& a, int splitk);
// The arguments of a launch on the GEMV layout (qweight int32 [N, K/8], qzeros int32 [N, ZW], scales fp16 [N, 8 ZW]) or the GEMVFast
// layout (qweight int16 [N/4, K], scales / qzeros fp16 [group_rows, N], qzeros = -(s z)): capi.hip checks what the C ABI passes,
// narrows the sizes and fills this once.  The layout is the launcher's; a kernel's tuning integers stay its launcher's parameters.
struct AwqGemvArgs {
    const uint16_t* x;       // [M, K] fp16 (the dequant launchers: not read)
    const void* qweight;     // the layout's packed words (awq_launch_gemm_regb_fz: GEMM-layout words [K, N/8], a repacked temporary)
    const uint16_t* scales;
    const void* qzeros;      // GEMV: packed zero nibbles; GEMVFast: fp16 zero terms
    uint16_t* y;             // [M, N] fp16 (the dequant launchers: W^T [N, K])
    int M, K, N, g;
    int width;               // GEMV: zeros_width ZW (words of zero nibbles per row); GEMVFast: group_rows (rows of scales / qzeros)
    hipStream_t stream;
};

// GEMV layout: MFMA GEMV, M <= 16, and the bit-exact dequant to W^T [N, K].  nwaves (4|8|16) / unroll (4|8): 0 = auto.
bool awq_gemv_nk_supports(int M, int K, int N, int g);
size_t awq_gemv_nk_lds_bytes(int M, int K, int ZW, int nwaves);
int awq_launch_gemv_nk(const AwqGemvArgs& a, int nwaves, int unroll);
// GEMV layout, row-streaming VALU kernel (gemv_rows.hip), M <= 4: waves per block (<= 8), super-units in flight per wave
// (1|2), blocks per CU, 1-KiB slots of a row per wave (1|2|3|4|6|8); 0 = auto each.
bool awq_gemv_rows_supports(int M, int K, int N, int g);
struct AwqRowsFx {  // decoder-block prologue / epilogue of the row-streaming kernel (batch 1): see awq_gemv_forward_ex
    const uint16_t* norm_w = nullptr;
    float norm_eps = 0.f;
    const uint16_t* res = nullptr;
    bool pairs = false;
    // grouped form (MoE decode): one virtual batch-1 call per (token, expert) pair over expert stacks [E, N, ...]; M must be 1,
    // x holds the activation rows (pair i reads row i / x_div), y [num_pairs, N (N / 2 with pairs)]
    const int32_t* pair_expert = nullptr;  // [num_pairs] on the device; a value outside [0, num_experts) skips the pair
    const float* pair_scale = nullptr;     // [num_pairs] routing weights folded into the epilogue, or null
    int num_pairs = 0, num_experts = 0, x_div = 1;
    int first_expert = 0;                  // pair_expert holds global ids; the stack holds experts [first_expert, first_expert + num_experts)
    int parts = 0;                         // blocks one expert matrix is dealt over (0 = auto)
};
int awq_launch_gemv_rows(const AwqGemvArgs& a, int waves, int depth, int bpc, int sl, const AwqRowsFx* fx = nullptr);
// GEMV layout, 2 <= M <= 16 while the activations fit LDS as MFMA fragments (M K <= 32768; M <= 8 at K = 4096): weights stream
// through LDS by DMA into v_mfma_f32_16x16x32_f16 (gemv_lds.hip).  ks: waves per tile (1|2|4), depth: pieces in flight; 0 = auto.
bool awq_gemv_lds_supports(int M, int K, int N, int g);
int awq_launch_gemv_lds(const AwqGemvArgs& a, int ks, int depth);
// GEMV layout, 1 <= M <= 32 per launch, group_size 128: activations as MFMA A fragments in registers, the K range of a 16-row tile
// split over the waves of one block, weights by LDS-DMA (gemv_batch.hip).  form: activations through a wave-private LDS staging area
// (1) or by direct fragment loads (2); depth: pieces in flight per wave (1..3); 0 = auto.
bool awq_gemv_batch_supports(int M, int K, int N, int g);
int awq_launch_gemv_batch(const AwqGemvArgs& a, int form, int depth);
// the same kernel on the GEMVFast layout's buffers (N % 16 == 0)
bool awq_gemv_batch_fast_supports(int M, int K, int N, int g);
int awq_launch_gemv_batch_fast(const AwqGemvArgs& a, int depth);
// host only: the plan of a launch (awq_gemv_batch_plan); false where the planner refuses the arguments
bool awq_gemv_batch_plan_fill(int M, int K, int N, int g, int form, int depth, bool fast, int32_t* out);
// GEMV layout, prefill-sized batches: the register-decoded MFMA GEMM reading the layout's own buffers (gemm_regb.hip, NK form)
bool awq_gemm_regb_nk_supports(int M, int K, int N, int g, int ZW);
int awq_launch_gemm_regb_nk(const AwqGemvArgs& a, int bm);
// GEMM-layout words + the GEMVFast format's scales / fp16 zero terms [>= K/g, N] (gemm_regb.hip, FZ form: W = fp16(w s + qzeros))
int awq_launch_gemm_regb_fz(const AwqGemvArgs& a, int bm);
// MoE prefill: the same kernel over a token list sorted by expert (device-side row offsets), GEMM-layout expert stacks; a.M = the pairs
int awq_launch_gemm_regb_grouped(const AwqGemmArgs& a, const AwqGroupedArgs& r, int bm);
int awq_launch_moe_sort(const int* ids, int P, int E, int* order, int* seg, hipStream_t st);
int awq_launch_dequant_nk(const AwqGemvArgs& a);
// Grouped (MoE) GEMM over stacked expert tensors (awq/modules/fused/moe.py:60-89), M = 16-row token blocks.
size_t awq_grouped_workspace_bytes_impl(int max_blocks, int K, int N);
int awq_launch_grouped_gemm(const AwqGemmArgs& a, const AwqGroupedArgs& r);
// out[r, d] = silu(in[r, d]) * in[r, D + d]   (awq_ext.silu_and_mul, moe.py:73-76)
int awq_launch_silu_and_mul(const uint16_t* in, uint16_t* out, int64_t rows, int64_t D, hipStream_t st);
// GEMVFast layout (qweight int16 [N/4, K], scales / qzeros fp16 [8*ZW, N], qzeros = -(s*z)).
bool awq_gemv_fast_supports(int M, int K, int N, int g);
size_t awq_gemv_fast_lds_bytes(int M, int K, int g, int nwaves);
int awq_launch_gemv_fast(const AwqGemvArgs& a, int nwaves, int unroll);
int awq_launch_dequant_fast(const AwqGemvArgs& a);
// MoE routing (softmax + top-k + block alignment) in one launch; T tokens, E <= 64 experts, k <= 8.
int awq_launch_moe_route(const float* logits, float* topk_w, int* topk_ids, int* sorted_ids, int* expert_ids,
                         int* num_post_pad, int T, int E, int k, int renorm, int block, int first_expert, int num_local,
                         hipStream_t st);

// decoder.hip: RMSNorm (+ residual add when `residual` is non-null), RoPE + KV-cache append, single-query attention
int awq_launch_rmsnorm(const uint16_t* x, uint16_t* residual, const uint16_t* w, uint16_t* out, int64_t M, int64_t H,
                       float eps, hipStream_t st);
// The arguments of the RoPE + append launch, as the C ABI passes them (the launcher narrows the sizes after capi.hip's range checks).
struct AwqAppendArgs {
    const uint16_t* qkv;  // [B, S, (Hq + 2 Hkv) D] fp16
    uint16_t* q_out;      // [B, S, Hq, D]
    void *k_cache, *v_cache;                      // [>= B, Tmax, Hkv, D]: fp16 rows, or e4m3 codes with
    float *k_scale = nullptr, *v_scale = nullptr;  // their scales [>= B, Tmax, Hkv] (null: an fp16 cache)
    const float *cos_t, *sin_t;
    const int32_t* pos_dev = nullptr;  // device position word: one for the batch, or [B] with `rows`; null: start_pos
    bool rows = false;
    const int32_t* count_dev = nullptr;  // with `rows`: [B] new tokens per sequence -- slots s >= count_dev[b] write nothing
    int64_t start_pos = 0, B, S, Hq, Hkv, D, rot, Tmax;
    hipStream_t stream;
};
int awq_launch_rope_kv_append(const AwqAppendArgs& a);

// The arguments of the decode-attention launch (and, with a token count, of the verify launch), as the C ABI passes them.
struct AwqAttnArgs {
    const uint16_t* q;  // query rows [B, Hq, D]; fused form: the raw qkv rows [B, (Hq + 2 Hkv) D]
    const void *k_cache, *v_cache;                       // [>= B, Tmax, Hkv, D]: fp16 rows, or e4m3 codes with
    const float *k_scale = nullptr, *v_scale = nullptr;  // their scales [>= B, Tmax, Hkv] (null: an fp16 cache).  The fused form
                                                         // WRITES the new token's row of all four
    uint16_t* out;                                 // [B, Hq, D]
    const int32_t* len_dev = nullptr;  // device length word (fused form: the POSITION of the new token): one for the batch, or [B]
    bool rows = false;                 // with `rows`; null: seq_len
    int64_t seq_len = 0;               // host length (fused form: position), read where len_dev is null
    int64_t max_len, B, Hq, Hkv, D, Tmax;  // max_len: the bound of the device word that the split is sized for
    float scale, softcap = 0.f;
    const float* alibi = nullptr;                     // slopes [Hq], or null
    const float *cos_t = nullptr, *sin_t = nullptr;  // non-null: the fused form (rotate q / k, append k / v, attend)
    void* workspace;
    size_t workspace_bytes;
    hipStream_t stream;
};
size_t awq_decode_attention_workspace_bytes_impl(int B, int Hq, int max_splits);
int awq_launch_decode_attention(const AwqAttnArgs& a);

// Splits per KV head of the decode and verify launches: about 128 rows each (AWQ_ATTN_ROWS; A/B on the whole-model decode,
// profiles/r04_attention_split_ab.txt: 128 rows 769 / 712 / 663 tok/s at 64 / 512 / 2048 tokens of context, 256 rows 772 / 657 /
// 564, 64 rows 768 / 694 / 589), at most ~1024 blocks (AWQ_ATTN_BLOCKS) and 64 splits (the combine kernels' one-lane-per-split
// step).  ONE split up to AWQ_ATTN_SINGLE = 256 rows: no partials, no combine launch at all -- what a short context pays for a
// 32-way split sized for the whole cache was 9.5 + 5 us per layer (profiles/r03_whole_model_gemv_kernel_stats.txt); callers that
// know the context on the host (modules/fused/decode.py: one hipGraph per length bucket) pass the bucket's bound as max_len.
// (The constants are overridable in experiment builds: tools/attn_split_ab.py.)
#ifndef AWQ_ATTN_BLOCKS
#define AWQ_ATTN_BLOCKS 1024
#endif
#ifndef AWQ_ATTN_ROWS
#define AWQ_ATTN_ROWS 128
#endif
#ifndef AWQ_ATTN_SINGLE
#define AWQ_ATTN_SINGLE 256
#endif
// Host only.  len: the rows the launch is sized for; blocks_per_split: the blocks one split adds to the grid (decode: B Hkv,
// verify: B Hkv token groups).  A workspace of workspace_bytes (0 where there is none) that holds fewer than the rule's splits
// of bytes_per_split each limits the count to what fits; the defaults leave the rule alone.  blocks_per_split is 64-bit: the C ABI
// admits B and Hkv up to 65535 each, and their product does not fit an int.
static inline int awq_attn_splits(int len, int64_t blocks_per_split, size_t workspace_bytes = SIZE_MAX, size_t bytes_per_split = 1) {
    int splits = len <= AWQ_ATTN_SINGLE ? 1 : (len + AWQ_ATTN_ROWS - 1) / AWQ_ATTN_ROWS;
    const int by_blocks = AWQ_ATTN_BLOCKS / blocks_per_split > 1 ? (int)(AWQ_ATTN_BLOCKS / blocks_per_split) : 1;
    if (splits > by_blocks) splits = by_blocks;
    if (splits < 1) splits = 1;
    if (splits > 64) splits = 64;
    if (splits > 1 && workspace_bytes / bytes_per_split < (size_t)splits) {
        splits = (int)(workspace_bytes / bytes_per_split);
        if (splits < 1) splits = 1;
    }
    return splits;
}

// fp8 KV cache (k_scale / v_scale above non-NULL: the caches hold e4m3 codes): fp16 rows <-> codes + scales
int awq_launch_kv_quant_fp8(const uint16_t* x, uint8_t* codes, float* scales, int B, int S, int Hkv, int Tmax, int start,
                            hipStream_t st);
int awq_launch_kv_dequant_fp8(const uint8_t* codes, const float* scales, uint16_t* out, int B, int n, int Hkv, int Tmax,
                              hipStream_t st);

// verify_attn.hip: attention of T = 2 .. 8 new tokens per sequence over the cache at per-row device positions (speculative decoding)
int awq_verify_attention_splits_impl(int max_len, int B, int T, int Hq, int Hkv);
size_t awq_verify_attention_workspace_bytes_impl(int B, int T, int Hq, int splits);
// (a: an fp16 cache, the per-row word and max_len; seq_len, softcap, alibi and the tables are not read)
int awq_launch_verify_attention(const AwqAttnArgs& a, int T);

// logprob.hip: log-probability of one id per row of fp16 logits, one block per row (capi.hip checks the arguments)
int awq_launch_token_logprobs(const AwqLogprobArgs& a);
