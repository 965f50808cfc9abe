// capi.hip -- the extern "C" surface of libawq_hip.so (declared in include/awq_hip.h).
// Validation + kernel selection only; kernels live in the other translation units.
#include "awq_internal.h"

/* ---- GEMM layout and the MoE grouped GEMMs built on it: an entry point checks what only it takes, calls check_gemm (the shape rule,
 * the ranges, the five operand pointers and their alignment; it fills the launch's arguments), and launches -- awq_gemm_forward and
 * its fused forms what gemm_plan names */
namespace {
thread_local const char* g_last_kernel = "none";

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The block tile the NLOG field asks of the LDS-tiled and register-decoded kernels: 2 = 256, 1 = 128 where the entry point takes
// both (`both`), anything else 0 = the launcher's choice.
inline int block_width(uint32_t flags, bool both) {
    const unsigned nlog = AWQ_GEMM_FLAG_NLOG(flags);
    return nlog == 2 ? 256 : (both && nlog == 1 ? 128 : 0);
}

// awq/modules/linear/gemm.py:132-133
bool gemm_layout(int64_t K, int64_t N, int64_t g) { return K >= 0 && N >= 0 && g > 0 && N % 8 == 0 && K % g == 0 && K <= INT32_MAX && N <= INT32_MAX; }

// The layout rule and the range of M; then, unless the call is empty (`empty`: the entry point's own rule -- the caller returns AWQ_OK),
// the five operand pointers and their 16-byte alignment.  own_range / own_present: the entry point's verdict on the sizes and
// pointers only it takes (its range checks answer AWQ_ERR_BAD_SHAPE like the rule; what it refuses with AWQ_ERR_UNSUPPORTED comes
// after).  The one place where the sizes are narrowed and the operands filled: the other fields of *a stay as they are.
int check_gemm(AwqGemmArgs* a, const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, uint16_t* y,
               int64_t M, int64_t K, int64_t N, int64_t g, void* stream, bool empty, bool own_range = true, bool own_present = true) {
    if (!gemm_layout(K, N, g) || M < 0 || M > INT32_MAX || !own_range) return AWQ_ERR_BAD_SHAPE;
    a->x = x; a->qweight = qweight; a->scales = scales; a->qzeros = qzeros; a->y = y;
    a->M = (int)M; a->K = (int)K; a->N = (int)N; a->g = (int)g;
    a->stream = static_cast<hipStream_t>(stream);
    if (empty) return AWQ_OK;
    if (!x || !qweight || !scales || !qzeros || !y || !own_present) return AWQ_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(scales) || !aligned16(qzeros) || !aligned16(y)) return AWQ_ERR_BAD_ALIGNMENT;
    return AWQ_OK;
}

// workspace = [control AWQ_WS_COUNTER_BYTES][exchange region E][scratch region E]; the grouped call has no scratch half
size_t region_bytes(int64_t M, int64_t N) {
    const int64_t m = M < 16 ? M : 16;
    size_t e = (size_t)(64 * m * (N + 512)) * 4;  // up to 64 slabs of [min(M,16), N rounded up to a tile]
    if (e > ((size_t)32 << 20)) e = (size_t)32 << 20;  // the launchers lower the split to what fits
    return (e + 255) & ~(size_t)255;
}

void carve_workspace(AwqGemmArgs* a, void* workspace, size_t bytes, bool scratch) {
    if (!workspace || bytes <= AWQ_WS_COUNTER_BYTES + (scratch ? 512u : 0u)) return;
    char* regions = static_cast<char*>(workspace) + AWQ_WS_COUNTER_BYTES;
    const size_t e = scratch ? ((bytes - AWQ_WS_COUNTER_BYTES) / 2) & ~(size_t)255 : bytes - AWQ_WS_COUNTER_BYTES;
    a->counters = static_cast<int*>(workspace);
    a->exchange = reinterpret_cast<float*>(regions);
    a->exchange_bytes = e;
    if (!scratch) return;
    a->partial = reinterpret_cast<float*>(regions + e);
    a->partial_floats = e / sizeof(float);
}

// The dispatch of awq_gemm_forward and its fused forms (host only, no launch): the kernel a call asks for FIRST -- the one it names,
// or AUTO's choice.  fused: gated activations or a _normed / _ex call (the decode kernel alone; the caller has checked that it takes
// the shape).  AUTO:
//  - 9 .. 16 rows of a plain call: the register-decoded batched kernel where it is already ahead of the decode kernel -- matrices of
//    up to 8191 rows and fewer than 64 column tiles (r02: 13.8 vs 15.6 us at 4096 x 11008, M = 16);
//  - up to 16 rows otherwise: the decode kernel; the naive kernel for the odd shapes it refuses;
//  - up to 64 rows: the batched kernel where it takes the shape;
//  - the register-decoded prefill kernel once its 128 x 256 tiles give every CU a block (r02 sweep, profiles/r02_regb_by_m.txt:
//    4096 x 11008 from M = 768, 11008 x 4096 from M = 2048); below that the LDS-tiled kernel with split-K (smaller tiles, in-launch
//    combine) fills the chip better; the naive kernel for odd shapes.
// Two choices can still fall through at run time, on their launcher's answer: see gemm_forward.
unsigned gemm_plan(unsigned kern, int M, int K, int N, int g, bool fused) {
    if (kern != AWQ_GEMM_KERNEL_AUTO) return kern;
    if (!fused && M >= 9 && M <= 16 && K < 8192 && (N + 255) / 256 < 64 && awq_gemm_skinny_supports(M, K, N, g)) return AWQ_GEMM_KERNEL_SKINNY;
    if (M <= 16) return awq_gemv_mfma_supports(M, K, N, g, 2) ? AWQ_GEMM_KERNEL_MFMA_GEMV : AWQ_GEMM_KERNEL_NAIVE;
    if (M <= 64 && awq_gemm_skinny_supports(M, K, N, g)) return AWQ_GEMM_KERNEL_SKINNY;
    if (awq_gemm_regb_supports(M, K, N, g) && (int64_t)((M + 127) / 128) * ((N + 255) / 256) >= 256) return AWQ_GEMM_KERNEL_REGB;
    return awq_gemm_tiled_supports(M, K, N, g) ? AWQ_GEMM_KERNEL_TILED : AWQ_GEMM_KERNEL_NAIVE;
}

// awq_gemm_forward, _normed and _ex: the C ABI's arguments travel in the published struct.  extras: a _normed / _ex call -- the
// decode kernel only, in-launch combine only -- whether or not it carries a norm weight (an _ex call with add_residual or ssq_out
// alone sets no gated mode and is restricted all the same).
int gemm_forward(const AwqGemmEx& e, bool extras) {
    const uint32_t flags = e.flags;
    const bool empty = e.M == 0 || e.N == 0;
    AwqGemmArgs a;
    int rc = check_gemm(&a, e.x, e.qweight, e.scales, e.qzeros, e.y, e.M, e.K, e.N, e.group_size, e.stream, empty);
    if (rc || empty) return rc;
    if (e.workspace && !aligned16(e.workspace)) return AWQ_ERR_BAD_ALIGNMENT;
    a.bias = e.bias;
    carve_workspace(&a, e.workspace, e.workspace_bytes, true);

    a.x_gated = (flags & AWQ_GEMM_FLAG_X_GATED_SILU) ? 1 : 0;
    if (e.norm_weight) {
        if (a.x_gated) return AWQ_ERR_UNSUPPORTED;
        a.x_gated = 2;
        a.res_in = e.residual_in; a.res_out = e.residual_out; a.norm_w = e.norm_weight; a.norm_eps = e.norm_eps;
        a.ssq_in = e.ssq_in; a.ssq_in_tiles = (int)e.ssq_in_tiles;
    }
    a.add_res = e.add_residual; a.ssq_out = e.ssq_out;
    const bool fused = a.x_gated || extras;
    const unsigned asked = AWQ_GEMM_FLAG_KERNEL(flags);
    if (fused && (a.M > 16 || !awq_gemv_mfma_supports(a.M, a.K, a.N, a.g, 2))) return AWQ_ERR_UNSUPPORTED;
    if (extras && (a.M > 4 || (flags & AWQ_GEMM_FLAG_TWO_PASS))) return AWQ_ERR_UNSUPPORTED;
    if (fused && asked != AWQ_GEMM_KERNEL_AUTO && asked != AWQ_GEMM_KERNEL_MFMA_GEMV) return AWQ_ERR_UNSUPPORTED;
    if (extras && AWQ_GEMM_FLAG_NLOG(flags) == 4) return AWQ_ERR_UNSUPPORTED;  // the epilogue assumes 256-column tiles
    int nlog = (int)AWQ_GEMM_FLAG_NLOG(flags);
    int splitk = (int)AWQ_GEMM_FLAG_SPLITK(flags);
    if ((int64_t)a.K * a.N / 2 >= ((int64_t)1 << 31)) return AWQ_ERR_UNSUPPORTED;  // 32-bit buffer offsets

    unsigned kern = gemm_plan(asked, a.M, a.K, a.N, a.g, fused);
    if (asked == AWQ_GEMM_KERNEL_AUTO && kern == AWQ_GEMM_KERNEL_MFMA_GEMV) {  // (the tuning bits are a named kernel's)
        rc = awq_launch_gemv_mfma(a, 0, 0, 0, 0, false);
        if (rc != AWQ_ERR_UNSUPPORTED) {
            g_last_kernel = "gemv_mfma";
            return rc;
        }
        if (fused) return AWQ_ERR_UNSUPPORTED;
        kern = AWQ_GEMM_KERNEL_NAIVE;  // M <= 16 that the decode launcher refused: odd shapes
    }
    switch (kern) {
        case AWQ_GEMM_KERNEL_NAIVE:
            g_last_kernel = "naive";
            return awq_launch_gemm_naive(a);
        case AWQ_GEMM_KERNEL_VALU: {
            if (nlog == 0) nlog = 3;
            if (splitk == 0) splitk = awq_gemv_valu_default_split(a.K, a.N, nlog);
            while (splitk > 1 && (size_t)splitk * a.M * a.N * 4 > a.partial_floats * sizeof(float)) --splitk;
            g_last_kernel = "gemv_valu";
            return awq_launch_gemv_valu(a, nlog, splitk, (flags & AWQ_GEMM_FLAG_NO_NT) == 0);
        }
        case AWQ_GEMM_KERNEL_MFMA_GEMV: {
            if (a.M > 16) return AWQ_ERR_UNSUPPORTED;
            g_last_kernel = "gemv_mfma";
            return awq_launch_gemv_mfma(a, nlog, (int)AWQ_GEMM_FLAG_WAVES(flags), (int)AWQ_GEMM_FLAG_UNIT(flags), splitk,
                                        (flags & AWQ_GEMM_FLAG_TWO_PASS) != 0);
        }
        case AWQ_GEMM_KERNEL_TILED:
            g_last_kernel = "gemm_tiled";
            return awq_launch_gemm_tiled(a, block_width(flags, true), splitk);
        case AWQ_GEMM_KERNEL_SKINNY: {
            rc = awq_launch_gemm_skinny(a, splitk);
            if (rc != AWQ_ERR_UNSUPPORTED || asked != AWQ_GEMM_KERNEL_AUTO || !awq_gemm_tiled_supports(a.M, a.K, a.N, a.g)) {
                g_last_kernel = "gemm_skinny";
                return rc;
            }
            g_last_kernel = "gemm_tiled";  // AUTO: a slice that does not fit (very wide matrices at M > 32): the LDS-tiled kernel
            return awq_launch_gemm_tiled(a, 0, 0);
        }
        case AWQ_GEMM_KERNEL_REGB:
            g_last_kernel = "gemm_regb";
            return awq_launch_gemm_regb(a, block_width(flags, true));
        default:
            return AWQ_ERR_UNSUPPORTED;
    }
}

// awq_grouped_gemm_prefill and _ex.  ex: the flag bits and x_div are validated, and the gather / scatter bits read (the plain entry
// looks at the tile-height field alone: as published)
int grouped_prefill(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, uint16_t* y,
                    const int32_t* seg_offsets, const int32_t* row_map, const float* pair_weights, int64_t P, int64_t x_div,
                    int64_t num_experts, int64_t K, int64_t N, int64_t group_size, uint32_t flags, void* stream, bool ex) {
    AwqGroupedArgs r;
    r.seg = seg_offsets; r.row_map = row_map; r.pair_weights = pair_weights;
    r.gather = ex && (flags & AWQ_GROUPED_PREFILL_GATHER_X); r.scatter = ex && (flags & AWQ_GROUPED_PREFILL_SCATTER_Y);
    const bool empty = P == 0 || N == 0;
    AwqGemmArgs a;
    const int rc = check_gemm(&a, x, qweight, scales, qzeros, y, P, K, N, group_size, stream, empty,
                              num_experts >= 1 && num_experts <= 4096 &&
                                  (!ex || (x_div >= 1 && !(flags & ~(0xF0u | AWQ_GROUPED_PREFILL_GATHER_X | AWQ_GROUPED_PREFILL_SCATTER_Y)))),
                              seg_offsets && (row_map || !(r.gather || r.scatter || pair_weights)));
    if (rc || empty) return rc;
    r.num_experts = (int)num_experts; r.x_div = (int)x_div;
    g_last_kernel = "gemm_regb_grouped";
    return awq_launch_gemm_regb_grouped(a, r, block_width(flags, false));
}
}  // namespace

extern "C" {

int awq_hip_abi_version(void) { return AWQ_HIP_ABI_VERSION; }

const char* awq_hip_error_string(int code) {
    switch (code) {
        case AWQ_OK: return "ok";
        case AWQ_ERR_BAD_SHAPE: return "bad shape (need N % 8 == 0, K % group_size == 0)";
        case AWQ_ERR_BAD_ALIGNMENT: return "pointer not 16-byte aligned";
        case AWQ_ERR_UNSUPPORTED: return "no kernel for this shape/variant";
        case AWQ_ERR_WORKSPACE: return "workspace missing or too small";
        case AWQ_ERR_LAUNCH: return "HIP launch error";
        case AWQ_ERR_NULL: return "required pointer is NULL";
        default: return "unknown error";
    }
}

const char* awq_hip_last_kernel(void) { return g_last_kernel; }

int awq_unpack_int4(const int32_t* q, uint8_t* out, int64_t rows, int64_t words, void* stream) {
    if (rows < 0 || words < 0) return AWQ_ERR_BAD_SHAPE;
    if (rows * words == 0) return AWQ_OK;
    if (!q || !out) return AWQ_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(out) & 7u) || (reinterpret_cast<uintptr_t>(q) & 3u)) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_unpack(q, out, rows, words, static_cast<hipStream_t>(stream));
}

// (no activations, and of the alignments only scales' and out's are looked at: the layout rule is all it shares with check_gemm)
int awq_dequantize_weights(const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, uint16_t* out,
                           int64_t K, int64_t N, int64_t group_size, void* stream) {
    if (!gemm_layout(K, N, group_size)) return AWQ_ERR_BAD_SHAPE;
    if (K * N == 0) return AWQ_OK;
    if (!qweight || !scales || !qzeros || !out) return AWQ_ERR_NULL;
    if (!aligned16(scales) || !aligned16(out)) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_dequant(qweight, scales, qzeros, out, K, N, group_size, static_cast<hipStream_t>(stream));
}

size_t awq_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size) {
    (void)group_size;
    if (M <= 0 || K <= 0 || N <= 0) return 0;
    return (size_t)AWQ_WS_COUNTER_BYTES + 2 * region_bytes(M, N);
}

int awq_gemm_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace) return AWQ_ERR_NULL;
    if (workspace_bytes < AWQ_WS_COUNTER_BYTES) return AWQ_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(workspace, 0, AWQ_WS_COUNTER_BYTES, st) != hipSuccess) return AWQ_ERR_LAUNCH;
    if (workspace_bytes > AWQ_WS_COUNTER_BYTES &&
        hipMemsetAsync(static_cast<char*>(workspace) + AWQ_WS_COUNTER_BYTES, 0xFF, workspace_bytes - AWQ_WS_COUNTER_BYTES, st) != hipSuccess)
        return AWQ_ERR_LAUNCH;
    return AWQ_OK;
}

int awq_gemm_forward(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                     const uint16_t* bias, uint16_t* y, int64_t M, int64_t K, int64_t N, int64_t group_size,
                     void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
    AwqGemmEx e{};
    e.flags = flags;
    e.x = x; e.qweight = qweight; e.scales = scales; e.qzeros = qzeros; e.bias = bias; e.y = y;
    e.M = M; e.K = K; e.N = N; e.group_size = group_size;
    e.workspace = workspace; e.workspace_bytes = workspace_bytes; e.stream = stream;
    return gemm_forward(e, false);
}

// its own checks come before the shape rule: as published
int awq_gemm_forward_normed(const uint16_t* x, const uint16_t* residual_in, uint16_t* residual_out,
                            const uint16_t* norm_weight, float eps, const int32_t* qweight, const uint16_t* scales,
                            const int32_t* qzeros, const uint16_t* bias, uint16_t* y, int64_t M, int64_t K, int64_t N,
                            int64_t group_size, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
    if (!norm_weight) return AWQ_ERR_NULL;
    if ((residual_in == nullptr) != (residual_out == nullptr)) return AWQ_ERR_NULL;
    if (residual_in && residual_in == residual_out) return AWQ_ERR_BAD_ALIGNMENT;  // every block reads it, one block writes
    if (!aligned16(norm_weight) || (residual_in && (!aligned16(residual_in) || !aligned16(residual_out))))
        return AWQ_ERR_BAD_ALIGNMENT;
    if (M > 4 || (flags & AWQ_GEMM_FLAG_X_GATED_SILU)) return AWQ_ERR_UNSUPPORTED;
    AwqGemmEx e{};
    e.flags = flags;
    e.x = x; e.qweight = qweight; e.scales = scales; e.qzeros = qzeros; e.bias = bias; e.y = y;
    e.M = M; e.K = K; e.N = N; e.group_size = group_size;
    e.workspace = workspace; e.workspace_bytes = workspace_bytes; e.stream = stream;
    e.norm_weight = norm_weight; e.norm_eps = eps; e.residual_in = residual_in; e.residual_out = residual_out;
    return gemm_forward(e, true);
}

int64_t awq_gemm_ex_ssq_tiles(int64_t N) { return N > 0 ? (N + 255) / 256 : 0; }

// (aliasing residuals and a wrong struct_bytes answer AWQ_ERR_BAD_SHAPE here, a NULL struct AWQ_ERR_NULL: as published)
int awq_gemm_forward_ex(const AwqGemmEx* e) {
    if (!e) return AWQ_ERR_NULL;
    if (e->struct_bytes != sizeof(AwqGemmEx)) return AWQ_ERR_BAD_SHAPE;
    if ((e->residual_in == nullptr) != (e->residual_out == nullptr)) return AWQ_ERR_NULL;
    if (e->residual_in && (!e->norm_weight || e->residual_in == e->residual_out)) return AWQ_ERR_BAD_SHAPE;
    if (e->ssq_in && (!e->norm_weight || e->residual_in || e->ssq_in_tiles < 1 || e->ssq_in_tiles > 64)) return AWQ_ERR_BAD_SHAPE;
    if (e->add_residual && e->add_residual == e->y) return AWQ_ERR_BAD_SHAPE;  // other tiles' blocks may still read it
    const uint16_t* ptrs[] = {e->norm_weight, e->residual_in, e->residual_out, e->add_residual};
    for (const uint16_t* q : ptrs)
        if (q && !aligned16(q)) return AWQ_ERR_BAD_ALIGNMENT;
    return gemm_forward(*e, true);
}

// Which kernel awq_gemm_forward's AUTO dispatch takes first for a plain call (gemm_plan).  -1: an invalid shape.
int awq_gemm_auto_kernel(int64_t M, int64_t K, int64_t N, int64_t group_size) {
    if (M <= 0 || K <= 0 || N <= 0 || M > INT32_MAX || !gemm_layout(K, N, group_size)) return -1;
    return (int)gemm_plan(AWQ_GEMM_KERNEL_AUTO, (int)M, (int)K, (int)N, (int)group_size, false);
}

int awq_gemm_workspace_status(const void* workspace, void* stream, int32_t* err_out) {
    if (!workspace || !err_out) return AWQ_ERR_NULL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t word = 0;
    if (hipMemcpyAsync(&word, workspace, sizeof(word), hipMemcpyDeviceToHost, st) != hipSuccess) return AWQ_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return AWQ_ERR_LAUNCH;
    *err_out = word;
    return AWQ_OK;
}

/* ---- fused MLP / MoE ------------------------------------------------------------------- */

int awq_silu_and_mul(const uint16_t* gate_up, uint16_t* out, int64_t rows, int64_t d, void* stream) {
    if (rows < 0 || d < 0 || d % 8) return AWQ_ERR_BAD_SHAPE;
    if (rows * d == 0) return AWQ_OK;
    if (!gate_up || !out) return AWQ_ERR_NULL;
    if (!aligned16(gate_up) || !aligned16(out)) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_silu_and_mul(gate_up, out, rows, d, static_cast<hipStream_t>(stream));
}

int awq_moe_route_local(const float* gating_logits, float* topk_weights, int32_t* topk_ids, int32_t* sorted_token_ids,
                        int32_t* expert_ids, int32_t* num_tokens_post_padded, int64_t num_tokens, int64_t num_experts,
                        int64_t topk, int renormalize, int64_t block_rows, int64_t first_expert, int64_t num_local,
                        void* stream) {
    if (num_tokens < 0 || num_experts < 1 || topk < 1 || block_rows < 0) return AWQ_ERR_BAD_SHAPE;
    if (first_expert < 0 || num_local < 1 || first_expert + num_local > num_experts) return AWQ_ERR_BAD_SHAPE;
    if (num_tokens == 0) return AWQ_OK;
    // block_rows == 0: routing only (softmax, top-k, renormalisation) -- the three alignment outputs are not touched and may be NULL
    if (!gating_logits || !topk_weights || !topk_ids || (block_rows > 0 && (!sorted_token_ids || !expert_ids || !num_tokens_post_padded)))
        return AWQ_ERR_NULL;
    if (num_tokens * topk > (1 << 24)) return AWQ_ERR_UNSUPPORTED;
    return awq_launch_moe_route(gating_logits, topk_weights, topk_ids, sorted_token_ids, expert_ids,
                                num_tokens_post_padded, (int)num_tokens, (int)num_experts, (int)topk, renormalize,
                                (int)block_rows, (int)first_expert, (int)num_local, static_cast<hipStream_t>(stream));
}

int awq_moe_route(const float* gating_logits, float* topk_weights, int32_t* topk_ids, int32_t* sorted_token_ids,
                  int32_t* expert_ids, int32_t* num_tokens_post_padded, int64_t num_tokens, int64_t num_experts,
                  int64_t topk, int renormalize, int64_t block_rows, void* stream) {
    return awq_moe_route_local(gating_logits, topk_weights, topk_ids, sorted_token_ids, expert_ids, num_tokens_post_padded,
                               num_tokens, num_experts, topk, renormalize, block_rows, 0, num_experts, stream);
}

size_t awq_grouped_gemm_workspace_bytes(int64_t max_blocks, int64_t K, int64_t N) {
    if (max_blocks <= 0 || K <= 0 || N <= 0) return 0;
    return awq_grouped_workspace_bytes_impl((int)max_blocks, (int)K, (int)N);
}

int awq_grouped_gemm_forward(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                             uint16_t* y, const int32_t* sorted_token_ids, const int32_t* expert_ids,
                             const int32_t* num_tokens_post_padded, const float* pair_weights, int64_t num_pairs,
                             int64_t x_div, int64_t block_rows, int64_t max_blocks, int64_t num_experts, int64_t K,
                             int64_t N, int64_t group_size, void* workspace, size_t workspace_bytes, void* stream) {
    return awq_grouped_gemm_forward_ex(x, qweight, scales, qzeros, y, sorted_token_ids, expert_ids, num_tokens_post_padded,
                                       pair_weights, num_pairs, x_div, block_rows, max_blocks, num_experts, K, N, group_size,
                                       workspace, workspace_bytes, 0u, stream);
}

int awq_grouped_gemm_forward_ex(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                                uint16_t* y, const int32_t* sorted_token_ids, const int32_t* expert_ids,
                                const int32_t* num_tokens_post_padded, const float* pair_weights, int64_t num_pairs,
                                int64_t x_div, int64_t block_rows, int64_t max_blocks, int64_t num_experts, int64_t K,
                                int64_t N, int64_t group_size, void* workspace, size_t workspace_bytes, uint32_t flags,
                                void* stream) {
    if (flags & ~AWQ_GEMM_FLAG_X_GATED_SILU) return AWQ_ERR_UNSUPPORTED;  // before anything else: as published
    const bool empty = num_pairs == 0 || max_blocks == 0 || N == 0;
    AwqGemmArgs a;  // M: the rows of a token block
    const int rc = check_gemm(&a, x, qweight, scales, qzeros, y, block_rows, K, N, group_size, stream, empty,
                              (block_rows == 8 || block_rows == 16) && num_pairs >= 0 && x_div >= 1 && max_blocks >= 0 && num_experts >= 1,
                              sorted_token_ids && expert_ids && num_tokens_post_padded);
    if (rc || empty) return rc;
    if ((int64_t)num_experts * K * N / 2 >= ((int64_t)1 << 40)) return AWQ_ERR_UNSUPPORTED;
    if ((int64_t)K * N / 2 >= ((int64_t)1 << 31)) return AWQ_ERR_UNSUPPORTED;
    a.x_gated = (flags & AWQ_GEMM_FLAG_X_GATED_SILU) ? 1 : 0;
    carve_workspace(&a, workspace, workspace_bytes, false);
    const int64_t NW = N / 8, G = K / group_size;
    AwqGroupedArgs r;
    r.sorted_ids = sorted_token_ids; r.expert_ids = expert_ids; r.num_post_pad = num_tokens_post_padded; r.pair_weights = pair_weights;
    r.num_pairs = (int)num_pairs; r.x_div = (int)x_div; r.max_blocks = (int)max_blocks;
    r.expert_qw_words = K * NW; r.expert_z_words = G * NW; r.expert_s_halfs = G * N;
    g_last_kernel = "gemv_mfma_grouped";
    return awq_launch_grouped_gemm(a, r);
}

int awq_grouped_gemm_prefill(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                             uint16_t* y, const int32_t* seg_offsets, int64_t P, int64_t num_experts, int64_t K, int64_t N,
                             int64_t group_size, uint32_t flags, void* stream) {
    return grouped_prefill(x, qweight, scales, qzeros, y, seg_offsets, nullptr, nullptr, P, 1, num_experts, K, N, group_size, flags,
                           stream, false);
}

int awq_moe_sort_pairs(const int32_t* topk_ids, int32_t* order, int32_t* seg_offsets, int64_t num_pairs, int64_t num_experts,
                       void* stream) {
    if (num_pairs < 0 || num_pairs > (1 << 24) || num_experts < 1) return AWQ_ERR_BAD_SHAPE;
    if (!seg_offsets || (num_pairs && (!topk_ids || !order))) return AWQ_ERR_NULL;
    if (num_experts > 64) return AWQ_ERR_UNSUPPORTED;
    if (num_pairs == 0) return hipMemsetAsync(seg_offsets, 0, (size_t)(num_experts + 1) * 4, static_cast<hipStream_t>(stream)) == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
    return awq_launch_moe_sort(topk_ids, (int)num_pairs, (int)num_experts, order, seg_offsets, static_cast<hipStream_t>(stream));
}

int awq_grouped_gemm_prefill_ex(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                                uint16_t* y, const int32_t* seg_offsets, const int32_t* row_map, const float* pair_weights,
                                int64_t P, int64_t x_div, int64_t num_experts, int64_t K, int64_t N, int64_t group_size,
                                uint32_t flags, void* stream) {
    return grouped_prefill(x, qweight, scales, qzeros, y, seg_offsets, row_map, pair_weights, P, x_div, num_experts, K, N, group_size,
                           flags, stream, true);
}

}  // extern "C"

/* ---- GEMV and GEMVFast layouts: an entry point checks what only it takes, calls its layout's checker (the shape rule, the required
 * pointers and their alignment; it fills the launch's arguments), asks the layout's dispatch what the call launches, and launches it */
namespace {
// the one place where the sizes are narrowed: after the checkers' range checks (the two dequantisers have none, as published)
AwqGemvArgs gemv_args(const uint16_t* x, const void* qweight, const uint16_t* scales, const void* qzeros, uint16_t* y, int64_t M,
                      int64_t K, int64_t N, int64_t g, int64_t width, void* stream) {
    return {x, qweight, scales, qzeros, y, (int)M, (int)K, (int)N, (int)g, (int)width, static_cast<hipStream_t>(stream)};
}

inline bool empty(const AwqGemvArgs& a) { return a.M == 0 || a.N == 0; }

// GEMV layout: the shape rule; then, unless the call is empty (the caller returns AWQ_OK on empty(*a)), the five pointers and the
// alignment of x, qweight and scales.  own_present / own_aligned: the entry point's verdict on the pointers only it takes or checks
// -- awq_gemv_forward looks at y's alignment for the PREFILL kernel alone, awq_gemv_forward_ex at its norm weight's, the grouped
// entry requires its pair list; nobody looks at qzeros'.  An entry point's own shape checks answer AWQ_ERR_BAD_SHAPE like the rule,
// so they run before this; what it refuses with AWQ_ERR_UNSUPPORTED (_ex: M != 1; grouped: its limits) comes after: as published.
int check_gemv(AwqGemvArgs* a, const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, uint16_t* y,
               int64_t M, int64_t K, int64_t N, int64_t g, int64_t ZW, void* stream, bool own_present = true, bool own_aligned = true) {
    if (K <= 0 || N < 0 || g <= 0 || K % g || K % 8 || ZW <= 0 || ZW * 8 < K / g) return AWQ_ERR_BAD_SHAPE;
    if (M < 0 || M > INT32_MAX || K > INT32_MAX || N > INT32_MAX) return AWQ_ERR_BAD_SHAPE;
    *a = gemv_args(x, qweight, scales, qzeros, y, M, K, N, g, ZW, stream);
    if (empty(*a)) return AWQ_OK;
    if (!x || !qweight || !scales || !qzeros || !y || !own_present) return AWQ_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(scales) || !own_aligned) return AWQ_ERR_BAD_ALIGNMENT;
    return AWQ_OK;
}

// GEMVFast layout: as above; qzeros (fp16 terms here) is aligned too.  awq_gemv_fast_prefill: own_* = its temporary and y.
int check_gemv_fast(AwqGemvArgs* a, const uint16_t* x, const int16_t* qweight, const uint16_t* scales, const uint16_t* qzeros,
                    uint16_t* y, int64_t M, int64_t K, int64_t N, int64_t g, int64_t group_rows, void* stream, bool own_present = true,
                    bool own_aligned = true) {
    if (K <= 0 || N < 0 || g <= 0 || K % g || N % 4 || K % 64 || group_rows < K / g) return AWQ_ERR_BAD_SHAPE;
    if (M < 0 || M > INT32_MAX || K > INT32_MAX || N > INT32_MAX) return AWQ_ERR_BAD_SHAPE;
    *a = gemv_args(x, qweight, scales, qzeros, y, M, K, N, g, group_rows, stream);
    if (empty(*a)) return AWQ_OK;
    if (!x || !qweight || !scales || !qzeros || !y || !own_present) return AWQ_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(scales) || !aligned16(qzeros) || !own_aligned) return AWQ_ERR_BAD_ALIGNMENT;
    return AWQ_OK;
}

// What a call launches: the kernel (-1: none takes it, AWQ_ERR_UNSUPPORTED) and, for the batched kernel, the rows per launch.
struct GemvPlan { int kernel, rows; };
const GemvPlan no_kernel{-1, 0};

// The batched kernel (gemv_batch.hip) runs any M in launches of at most 128 rows (up to four row parts of <= 32 rows, each in its
// own block, the blocks of a tile list residents of one XCD so that the matrix is fetched from HBM once); where the parts do not fit
// the LDS budget (very long tile lists per block) launches of fewer rows.  The rows per launch, balanced; 0: the kernel refuses.
int batch_rows(bool (*supports)(int, int, int, int), int M, int K, int N, int g) {
    int cap = 128;
    while (cap > 32 && !supports(M > cap ? cap : M, K, N, g)) cap /= 2;
    if (!supports(M > cap ? cap : M, K, N, g)) return 0;
    const int nchunk = (M + cap - 1) / cap;
    return (M + nchunk - 1) / nchunk;
}

template <class Launch>
int launch_row_chunks(const AwqGemvArgs& a, int rows, Launch launch) {
    for (int64_t m0 = 0; m0 < a.M; m0 += rows) {
        AwqGemvArgs c = a;
        c.x += m0 * a.K, c.y += m0 * a.N;
        c.M = (int)(a.M - m0 < rows ? a.M - m0 : rows);
        if (const int rc = launch(c)) return rc;
    }
    return AWQ_OK;
}

// The dispatch of awq_gemv_forward (host only, no launch).  AUTO:
//  - the batched kernel (activations in registers, the K range split over the waves of a block, weights by LDS-DMA) wherever it
//    takes the shape (group_size 128) from five rows, four while K > 2048, three where the row-streaming kernel is not the choice
//    (K > 6144): it costs the same at 1 .. 5 rows while gemv_rows / gemv_nk grow by ~1 us per row
//    (profiles/r05_sweep_small_batch.txt, M = 4: 9.1 vs 10.3 us at 4096 x 11008, 14.4 vs 15.3 at 4096 x 22016, 12.7 vs 17.6 at
//    8192 x 7168; level at K = 11008; behind at K = 1024); 4096 x 11008, M = 8: see profiles/r05_*;
//  - the row-streaming kernel at batches 1 and 2 and at batches 3 .. 4 while K <= 6144: ahead of the 16-row tile kernel there on
//    all four 7B shapes (profiles/r03_gemv_rows_sweep.txt: M = 2 4.65 / 7.05 / 10.77 / 8.57 us vs 6.18 / 9.96 / 16.65 / 10.73;
//    M = 4 at K = 4096 5.79 / 9.79 / 14.39 vs 6.59 / 10.40 / 18.29; at K = 11008 12.25 vs 11.79);
//  - the LDS-streaming MFMA kernel from five rows on matrices of 8192 rows and more (4096 x 11008, M = 8: 11.6 us vs 19.0 for the
//    tile kernel; 4096 x 22016: 16.7 vs 35.7; below that the tile kernel is level or ahead);
//  - the 16-row MFMA tile kernel otherwise.  PREFILL is explicit only.
// A kernel the caller names is not replaced where it refuses the shape (ROWS, LDS, BATCH: no kernel); a number that names none runs
// the tile kernel.  All but the batched kernel take at most 16 rows per call (the host wrapper chunks).
GemvPlan gemv_plan(uint32_t kern, int M, int K, int N, int g) {
    if (kern == AWQ_GEMV_KERNEL_PREFILL) return {(int)kern, M};
    if (kern == AWQ_GEMV_KERNEL_BATCH || (kern == AWQ_GEMV_KERNEL_AUTO && (M >= 5 || (M == 4 && K > 2048) || (M == 3 && K > 6144)) &&
                                          awq_gemv_batch_supports(M > 32 ? 32 : M, K, N, g))) {
        const int rows = batch_rows(awq_gemv_batch_supports, M, K, N, g);
        return rows ? GemvPlan{(int)AWQ_GEMV_KERNEL_BATCH, rows} : no_kernel;
    }
    if (M > 16) return no_kernel;
    if (kern == AWQ_GEMV_KERNEL_AUTO) {
        if ((M <= 2 || (M <= 4 && K <= 6144)) && awq_gemv_rows_supports(M, K, N, g)) kern = AWQ_GEMV_KERNEL_ROWS;
        else if (M >= 5 && N >= 8192 && awq_gemv_lds_supports(M, K, N, g)) kern = AWQ_GEMV_KERNEL_LDS;
    }
    if (kern == AWQ_GEMV_KERNEL_ROWS) return awq_gemv_rows_supports(M, K, N, g) ? GemvPlan{(int)kern, M} : no_kernel;
    if (kern == AWQ_GEMV_KERNEL_LDS) return awq_gemv_lds_supports(M, K, N, g) ? GemvPlan{(int)kern, M} : no_kernel;
    return awq_gemv_nk_supports(M, K, N, g) ? GemvPlan{(int)AWQ_GEMV_KERNEL_TILE16, M} : no_kernel;
}

// The dispatch of awq_gemv_fast_forward.  AUTO: the batched kernel (GEMVFast form) where it takes the shape, from five rows -- and
// below five where ONE pass of eight waves covers K (2048 < K <= 4096): there it is ahead of the 16-row kernel at every M
// (profiles/r05_sweep_small_batch.txt, M = 1: 5.4 / 9.3 / 9.6 / 15.0 us vs 6.2 / 9.7 / 10.1 / 16.3 at N = 4096 / 11008 / 12288 /
// 22016), behind it at K = 1024 (fewer waves per tile) and from K = 8192 (two passes).  Every number but 0 and BATCH: the 16-row
// kernel (gemv_fast.hip, M <= 16: the host wrapper chunks).
GemvPlan gemv_fast_plan(uint32_t kern, int M, int K, int N, int g) {
    const int rows = batch_rows(awq_gemv_batch_fast_supports, M, K, N, g);
    if (kern == AWQ_GEMV_KERNEL_BATCH || (kern == AWQ_GEMV_KERNEL_AUTO && (M >= 5 || (K > 2048 && K <= 4096)) && rows))
        return rows ? GemvPlan{(int)AWQ_GEMV_KERNEL_BATCH, rows} : no_kernel;
    return M <= 16 && awq_gemv_fast_supports(M, K, N, g) ? GemvPlan{(int)AWQ_GEMV_KERNEL_TILE16, M} : no_kernel;
}
}  // namespace

extern "C" {

// Which kernel awq_gemv_forward's AUTO dispatch takes (gemv_plan).  -1: no kernel takes the shape.
int awq_gemv_auto_kernel(int64_t M, int64_t K, int64_t N, int64_t group_size) {
    if (M <= 0 || K <= 0 || N <= 0 || group_size <= 0 || K % group_size || K % 8 || M > INT32_MAX || K > INT32_MAX || N > INT32_MAX) return -1;
    return gemv_plan(AWQ_GEMV_KERNEL_AUTO, (int)M, (int)K, (int)N, (int)group_size).kernel;
}

int awq_gemv_batch_plan(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t form, int32_t depth, int32_t fast, int32_t* out) {
    if (!out) return AWQ_ERR_NULL;
    if (M < 1 || M > 128 || K <= 0 || N <= 0 || group_size <= 0 || K > INT32_MAX || N > INT32_MAX || group_size > INT32_MAX) return AWQ_ERR_UNSUPPORTED;
    return awq_gemv_batch_plan_fill((int)M, (int)K, (int)N, (int)group_size, (int)form, (int)depth, fast != 0, out) ? AWQ_OK : AWQ_ERR_UNSUPPORTED;
}

int awq_gemv_forward(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                     uint16_t* y, int64_t M, int64_t K, int64_t N, int64_t group_size, int64_t zeros_width,
                     uint32_t flags, void* stream) {
    const uint32_t kern = AWQ_GEMM_FLAG_KERNEL(flags);
    AwqGemvArgs a;
    const int rc = check_gemv(&a, x, qweight, scales, qzeros, y, M, K, N, group_size, zeros_width, stream, true,
                              kern != AWQ_GEMV_KERNEL_PREFILL || aligned16(y));
    if (rc || empty(a)) return rc;
    const GemvPlan plan = gemv_plan(kern, a.M, a.K, a.N, a.g);
    const int waves = (int)AWQ_GEMM_FLAG_WAVES(flags), unit = (int)AWQ_GEMM_FLAG_UNIT(flags), split = (int)AWQ_GEMM_FLAG_SPLITK(flags);
    switch (plan.kernel) {
        case AWQ_GEMV_KERNEL_PREFILL:
            g_last_kernel = "gemm_regb_nk";
            return awq_launch_gemm_regb_nk(a, block_width(flags, false));
        case AWQ_GEMV_KERNEL_BATCH: {
            g_last_kernel = "gemv_batch";
            // the tuning bits are the batch kernel's only when the caller picked it: AUTO plans with 0 (flags written for another kernel
            // must not move the batch kernel's row parts / form / ring depth)
            const bool tuned = kern == AWQ_GEMV_KERNEL_BATCH;
            const int form = tuned ? unit | (waves << 4) : 0, depth = tuned ? split : 0;
            return launch_row_chunks(a, plan.rows, [&](const AwqGemvArgs& c) { return awq_launch_gemv_batch(c, form, depth); });
        }
        case AWQ_GEMV_KERNEL_ROWS:
            g_last_kernel = "gemv_rows";
            return awq_launch_gemv_rows(a, waves, unit, split, (int)AWQ_GEMM_FLAG_NLOG(flags));
        case AWQ_GEMV_KERNEL_LDS:
            g_last_kernel = "gemv_lds";
            return awq_launch_gemv_lds(a, split, unit);
        case AWQ_GEMV_KERNEL_TILE16:
            g_last_kernel = "gemv_nk";
            return awq_launch_gemv_nk(a, waves, unit);
        default:
            return AWQ_ERR_UNSUPPORTED;
    }
}

int awq_gemv_forward_ex(const AwqGemvEx* e) {
    if (!e || e->struct_bytes != sizeof(AwqGemvEx)) return AWQ_ERR_BAD_SHAPE;  // (a NULL struct too: as published)
    const bool pairs = e->flags & AWQ_GEMV_EX_SILU_PAIRS;
    if ((e->flags & ~AWQ_GEMV_EX_SILU_PAIRS) || (pairs && (e->add_residual || e->N % 2))) return AWQ_ERR_BAD_SHAPE;
    AwqGemvArgs a;
    const int rc = check_gemv(&a, e->x, e->qweight, e->scales, e->qzeros, e->y, e->M, e->K, e->N, e->group_size, e->zeros_width,
                              e->stream, true, !e->norm_weight || aligned16(e->norm_weight));
    if (rc || empty(a)) return rc;
    if (a.M != 1) return AWQ_ERR_UNSUPPORTED;
    const AwqRowsFx fx{e->norm_weight, e->norm_eps, e->add_residual, pairs};
    g_last_kernel = "gemv_rows";
    return awq_launch_gemv_rows(a, 0, 0, 0, 0, &fx);
}

int awq_grouped_gemv_forward(const uint16_t* x, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                             uint16_t* y, const int32_t* pair_experts, const float* pair_weights, int64_t num_pairs,
                             int64_t x_div, int64_t num_experts, int64_t first_expert, int64_t K, int64_t N, int64_t group_size,
                             int64_t zeros_width, uint32_t flags, int64_t parts, void* stream) {
    if (first_expert < 0 || first_expert > INT32_MAX) return AWQ_ERR_BAD_SHAPE;
    if (num_pairs < 0 || num_experts < 1 || num_experts > INT32_MAX || x_div < 1 || parts < 0 || (flags & ~AWQ_GEMV_EX_SILU_PAIRS))
        return AWQ_ERR_BAD_SHAPE;
    const bool pairs = flags & AWQ_GEMV_EX_SILU_PAIRS;
    if (pairs && (pair_weights || N % 2)) return AWQ_ERR_BAD_SHAPE;
    AwqGemvArgs a;
    // one virtual batch-1 call per pair (a count past the limit is refused below, not by the range of M)
    const int rc = check_gemv(&a, x, qweight, scales, qzeros, y, num_pairs ? 1 : 0, K, N, group_size, zeros_width, stream, pair_experts != nullptr);
    if (rc || empty(a)) return rc;
    // (the limits come after the pointer and alignment checks: as published)
    if (num_pairs > 8191 || parts > 65535 || x_div > num_pairs) return AWQ_ERR_UNSUPPORTED;
    // the per-expert strides must keep every expert's tensors 16-byte aligned (whole rows of 16-byte multiples)
    if ((N * (K / 8) * 4) % 16 || (N * zeros_width * 16) % 16) return AWQ_ERR_UNSUPPORTED;
    AwqRowsFx fx;
    fx.pairs = pairs; fx.pair_expert = pair_experts; fx.pair_scale = pair_weights;
    fx.num_pairs = (int)num_pairs; fx.num_experts = (int)num_experts; fx.first_expert = (int)first_expert;
    fx.x_div = (int)x_div; fx.parts = (int)parts;
    g_last_kernel = "gemv_rows_grouped";
    return awq_launch_gemv_rows(a, 0, 0, 0, 0, &fx);
}

size_t awq_gemv_lds_bytes(int64_t M, int64_t K, int64_t zeros_width) {
    return awq_gemv_nk_lds_bytes((int)M, (int)K, (int)zeros_width, 8);
}

// (the two dequantisers have looser shape rules than the forward entries -- no range, no width -- and check less alignment: as published)
int awq_dequantize_weights_gemv(const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, uint16_t* out,
                                int64_t K, int64_t N, int64_t group_size, int64_t zeros_width, void* stream) {
    if (K < 0 || N < 0 || group_size <= 0 || K % 8 || group_size % 8 || (K && K % group_size)) return AWQ_ERR_BAD_SHAPE;
    if (K * N == 0) return AWQ_OK;
    if (!qweight || !scales || !qzeros || !out) return AWQ_ERR_NULL;
    if (!aligned16(out)) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_dequant_nk(gemv_args(nullptr, qweight, scales, qzeros, out, 0, K, N, group_size, zeros_width, stream));
}

int awq_gemv_fast_forward(const uint16_t* x, const int16_t* qweight, const uint16_t* scales, const uint16_t* qzeros,
                          uint16_t* y, int64_t M, int64_t K, int64_t N, int64_t group_size, int64_t group_rows,
                          uint32_t flags, void* stream) {
    AwqGemvArgs a;
    const int rc = check_gemv_fast(&a, x, qweight, scales, qzeros, y, M, K, N, group_size, group_rows, stream);
    if (rc || empty(a)) return rc;
    const uint32_t kern = AWQ_GEMM_FLAG_KERNEL(flags);
    const GemvPlan plan = gemv_fast_plan(kern, a.M, a.K, a.N, a.g);
    if (plan.kernel == (int)AWQ_GEMV_KERNEL_BATCH) {
        g_last_kernel = "gemv_batch_fast";
        // (tuning bits only when the caller picked the batch kernel: AUTO plans with 0)
        const int depth = kern == AWQ_GEMV_KERNEL_BATCH ? (int)((AWQ_GEMM_FLAG_SPLITK(flags) & 15u) | (AWQ_GEMM_FLAG_WAVES(flags) << 4)) : 0;
        return launch_row_chunks(a, plan.rows, [&](const AwqGemvArgs& c) { return awq_launch_gemv_batch_fast(c, depth); });
    }
    if (plan.kernel < 0) return AWQ_ERR_UNSUPPORTED;
    g_last_kernel = "gemv_fast";
    return awq_launch_gemv_fast(a, (int)AWQ_GEMM_FLAG_WAVES(flags), (int)AWQ_GEMM_FLAG_UNIT(flags));
}

// Prefill-sized batches on the GEMVFast layout: the packed words are transposed into the caller's temporary (repack.hip), then the
// register-decoded MFMA GEMM runs on it with the format's own scales / fp16 zero terms (gemm_regb.hip, FZ form).  Two launches.
int awq_gemv_fast_prefill(const uint16_t* x, const int16_t* qweight, const uint16_t* scales, const uint16_t* qzeros, uint16_t* y,
                          int32_t* qweight_tmp, int64_t M, int64_t K, int64_t N, int64_t group_size, int64_t group_rows, uint32_t flags,
                          void* stream) {
    AwqGemvArgs a;
    int rc = check_gemv_fast(&a, x, qweight, scales, qzeros, y, M, K, N, group_size, group_rows, stream, qweight_tmp != nullptr,
                             aligned16(y) && aligned16(qweight_tmp));
    if (rc || empty(a)) return rc;
    if (N % 8 || !awq_gemm_regb_supports(a.M, a.K, a.N, a.g)) return AWQ_ERR_UNSUPPORTED;
    rc = awq_repack_gemvfast_to_gemm(qweight, qweight_tmp, K, N, stream);
    if (rc != AWQ_OK) return rc;
    g_last_kernel = "repack_fast+gemm_regb_fz";
    a.qweight = qweight_tmp;  // the GEMM runs on the transposed words
    return awq_launch_gemm_regb_fz(a, block_width(flags, false));
}

size_t awq_gemv_fast_lds_bytes_c(int64_t M, int64_t K, int64_t group_size) {
    return awq_gemv_fast_lds_bytes((int)M, (int)K, (int)group_size, 8);
}

int awq_dequantize_weights_gemv_fast(const int16_t* qweight, const uint16_t* scales, const uint16_t* qzeros,
                                     uint16_t* out, int64_t K, int64_t N, int64_t group_size, void* stream) {
    if (K < 0 || N < 0 || group_size <= 0 || K % 64 || N % 4 || (K && K % group_size)) return AWQ_ERR_BAD_SHAPE;
    if (K * N == 0) return AWQ_OK;
    if (!qweight || !scales || !qzeros || !out) return AWQ_ERR_NULL;
    return awq_launch_dequant_fast(gemv_args(nullptr, qweight, scales, qzeros, out, 0, K, N, group_size, 0, stream));
}

}  // extern "C"

// ---- fused decoder block (decoder.hip)
int awq_rmsnorm_forward(const uint16_t* x, uint16_t* residual, const uint16_t* weight, uint16_t* out, int64_t M, int64_t H,
                        float eps, void* stream) {
    if (M < 0 || H <= 0) return AWQ_ERR_BAD_SHAPE;
    if (M == 0) return AWQ_OK;
    if (!x || !weight || !out) return AWQ_ERR_NULL;
    if (!aligned16(x) || !aligned16(weight) || !aligned16(out) || (residual && !aligned16(residual))) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_rmsnorm(x, residual, weight, out, M, H, eps, static_cast<hipStream_t>(stream));
}

// ---- RoPE + append and decode attention (decoder.hip): an entry point fills the launch's arguments; one function per family
// checks them and launches.  The entry points of a family differ in what they require; the one place where they also differ in
// the order of two checks is noted at decode_attention below.

// fp8 KV cache (KV8): the caches, their scale arrays and head_dim == 128
static int kv8_check(const void* kc, const void* vc, const float* ks, const float* vs, int64_t head_dim) {
    if (!kc || !vc || !ks || !vs) return AWQ_ERR_NULL;
    if (head_dim != 128) return AWQ_ERR_UNSUPPORTED;
    if (!aligned16(kc) || !aligned16(vc) || (reinterpret_cast<uintptr_t>(ks) & 3) || (reinterpret_cast<uintptr_t>(vs) & 3))
        return AWQ_ERR_BAD_ALIGNMENT;
    return AWQ_OK;
}

// kv8: an *_fp8 entry (the scale arrays are required, and the caches are checked with them)
static int rope_kv_append(const AwqAppendArgs& a, bool kv8) {
    if (a.B < 0 || a.S < 0 || a.B * a.S > INT32_MAX / 1024 || a.Tmax < 1 || a.Tmax > INT32_MAX) return AWQ_ERR_BAD_SHAPE;
    if (a.B * a.S == 0) return AWQ_OK;
    if (!a.qkv || !a.q_out || (a.rows && !a.pos_dev) || (a.rot > 0 && (!a.cos_t || !a.sin_t))) return AWQ_ERR_NULL;
    if (kv8) {
        if (int rc = kv8_check(a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.D)) return rc;
    } else if (!a.k_cache || !a.v_cache) {
        return AWQ_ERR_NULL;
    }
    return awq_launch_rope_kv_append(a);
}

// kv8: as above.  rope: a fused entry -- the tables are required, and without a device word the host position (a.seq_len) must lie
// inside the cache.  The soft cap is checked for every entry: the ones that take none leave it 0.  An fp8 entry refuses a head
// size (kv8_check) BEFORE it looks at the alignment of q and out, an fp16 entry after (the launcher): kept as published.
static int decode_attention(const AwqAttnArgs& a, bool kv8, bool rope) {
    if (a.B < 0 || a.B > 65535 || a.Hq < 1 || a.Hkv < 1 || a.Hkv > 65535 || a.Tmax > INT32_MAX) return AWQ_ERR_BAD_SHAPE;
    if (!(a.softcap >= 0.f)) return AWQ_ERR_BAD_SHAPE;
    if (a.B == 0) return AWQ_OK;
    if (!a.q || !a.out || (a.rows && !a.len_dev) || (rope && (!a.cos_t || !a.sin_t))) return AWQ_ERR_NULL;
    if (kv8) {
        if (int rc = kv8_check(a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.D)) return rc;
    } else {
        if (!a.k_cache || !a.v_cache) return AWQ_ERR_NULL;
        if (!aligned16(a.k_cache) || !aligned16(a.v_cache)) return AWQ_ERR_BAD_ALIGNMENT;
    }
    if (!aligned16(a.q) || !aligned16(a.out)) return AWQ_ERR_BAD_ALIGNMENT;
    if (rope && !a.len_dev && (a.seq_len < 0 || a.seq_len >= a.Tmax)) return AWQ_ERR_BAD_SHAPE;
    return awq_launch_decode_attention(a);
}

int awq_rope_kv_append(const uint16_t* qkv, uint16_t* q_out, uint16_t* k_cache, uint16_t* v_cache, const float* cos_table,
                       const float* sin_table, const int32_t* pos_dev, int64_t start_pos, int64_t B, int64_t S,
                       int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t rotary_dim, int64_t max_seq,
                       void* stream) {
    AwqAppendArgs a;
    a.qkv = qkv, a.q_out = q_out, a.k_cache = k_cache, a.v_cache = v_cache, a.cos_t = cos_table, a.sin_t = sin_table;
    a.pos_dev = pos_dev, a.start_pos = start_pos;
    a.B = B, a.S = S, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.rot = rotary_dim, a.Tmax = max_seq;
    a.stream = static_cast<hipStream_t>(stream);
    return rope_kv_append(a, false);
}

int awq_rope_kv_append_rows(const uint16_t* qkv, uint16_t* q_out, uint16_t* k_cache, uint16_t* v_cache, const float* cos_table,
                            const float* sin_table, const int32_t* pos_rows, int64_t B, int64_t S, int64_t n_heads,
                            int64_t n_kv_heads, int64_t head_dim, int64_t rotary_dim, int64_t max_seq, void* stream) {
    AwqAppendArgs a;
    a.qkv = qkv, a.q_out = q_out, a.k_cache = k_cache, a.v_cache = v_cache, a.cos_t = cos_table, a.sin_t = sin_table;
    a.pos_dev = pos_rows, a.rows = true;
    a.B = B, a.S = S, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.rot = rotary_dim, a.Tmax = max_seq;
    a.stream = static_cast<hipStream_t>(stream);
    return rope_kv_append(a, false);
}

int awq_rope_kv_append_fp8(const uint16_t* qkv, uint16_t* q_out, uint8_t* k_cache, uint8_t* v_cache, float* k_scale, float* v_scale,
                           const float* cos_table, const float* sin_table, const int32_t* pos_dev, int64_t start_pos, int64_t B,
                           int64_t S, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t rotary_dim, int64_t max_seq,
                           void* stream) {
    AwqAppendArgs a;
    a.qkv = qkv, a.q_out = q_out, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale;
    a.cos_t = cos_table, a.sin_t = sin_table, a.pos_dev = pos_dev, a.start_pos = start_pos;
    a.B = B, a.S = S, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.rot = rotary_dim, a.Tmax = max_seq;
    a.stream = static_cast<hipStream_t>(stream);
    return rope_kv_append(a, true);
}

int awq_rope_kv_append_rows_fp8(const uint16_t* qkv, uint16_t* q_out, uint8_t* k_cache, uint8_t* v_cache, float* k_scale,
                                float* v_scale, const float* cos_table, const float* sin_table, const int32_t* pos_rows, int64_t B,
                                int64_t S, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t rotary_dim,
                                int64_t max_seq, void* stream) {
    AwqAppendArgs a;
    a.qkv = qkv, a.q_out = q_out, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale;
    a.cos_t = cos_table, a.sin_t = sin_table, a.pos_dev = pos_rows, a.rows = true;
    a.B = B, a.S = S, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.rot = rotary_dim, a.Tmax = max_seq;
    a.stream = static_cast<hipStream_t>(stream);
    return rope_kv_append(a, true);
}

int awq_rope_kv_append_rows_n(const uint16_t* qkv, uint16_t* q_out, uint16_t* k_cache, uint16_t* v_cache, const float* cos_table,
                              const float* sin_table, const int32_t* pos_rows, const int32_t* count_rows, int64_t B, int64_t S,
                              int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t rotary_dim, int64_t max_seq, void* stream) {
    AwqAppendArgs a;
    a.qkv = qkv, a.q_out = q_out, a.k_cache = k_cache, a.v_cache = v_cache, a.cos_t = cos_table, a.sin_t = sin_table;
    a.pos_dev = pos_rows, a.rows = true, a.count_dev = count_rows;
    a.B = B, a.S = S, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.rot = rotary_dim, a.Tmax = max_seq;
    a.stream = static_cast<hipStream_t>(stream);
    if (B > 0 && S > 0 && !count_rows) return AWQ_ERR_NULL;
    return rope_kv_append(a, false);
}

int awq_rope_kv_append_rows_n_fp8(const uint16_t* qkv, uint16_t* q_out, uint8_t* k_cache, uint8_t* v_cache, float* k_scale,
                                  float* v_scale, const float* cos_table, const float* sin_table, const int32_t* pos_rows,
                                  const int32_t* count_rows, int64_t B, int64_t S, int64_t n_heads, int64_t n_kv_heads,
                                  int64_t head_dim, int64_t rotary_dim, int64_t max_seq, void* stream) {
    AwqAppendArgs a;
    a.qkv = qkv, a.q_out = q_out, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale;
    a.cos_t = cos_table, a.sin_t = sin_table, a.pos_dev = pos_rows, a.rows = true, a.count_dev = count_rows;
    a.B = B, a.S = S, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.rot = rotary_dim, a.Tmax = max_seq;
    a.stream = static_cast<hipStream_t>(stream);
    if (B > 0 && S > 0 && !count_rows) return AWQ_ERR_NULL;
    return rope_kv_append(a, true);
}

size_t awq_decode_attention_workspace_bytes(int64_t B, int64_t n_heads) {
    if (B <= 0 || n_heads <= 0) return 0;
    return awq_decode_attention_workspace_bytes_impl((int)B, (int)n_heads, 64);
}

int awq_decode_attention_ex(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, uint16_t* out,
                            const int32_t* len_dev, int64_t seq_len, int64_t max_len, int64_t B, int64_t n_heads,
                            int64_t n_kv_heads, int64_t head_dim, int64_t max_seq, float scale, float softcap,
                            const float* alibi_slopes, void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = q, a.k_cache = k_cache, a.v_cache = v_cache, a.out = out, a.len_dev = len_dev, a.seq_len = seq_len, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.softcap = softcap, a.alibi = alibi_slopes;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, false, false);
}

int awq_decode_attention(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, uint16_t* out,
                         const int32_t* len_dev, int64_t seq_len, int64_t max_len, int64_t B, int64_t n_heads,
                         int64_t n_kv_heads, int64_t head_dim, int64_t max_seq, float scale, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return awq_decode_attention_ex(q, k_cache, v_cache, out, len_dev, seq_len, max_len, B, n_heads, n_kv_heads, head_dim, max_seq,
                                   scale, 0.f, nullptr, workspace, workspace_bytes, stream);
}

int awq_decode_attention_rope(const uint16_t* qkv, uint16_t* k_cache, uint16_t* v_cache, const float* cos_table,
                              const float* sin_table, uint16_t* out, const int32_t* pos_dev, int64_t start_pos,
                              int64_t max_len, int64_t B, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                              int64_t max_seq, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = qkv, a.k_cache = k_cache, a.v_cache = v_cache, a.out = out, a.len_dev = pos_dev, a.seq_len = start_pos, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.cos_t = cos_table, a.sin_t = sin_table;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, false, true);
}

int awq_decode_attention_rows(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, uint16_t* out,
                              const int32_t* len_rows, int64_t max_len, int64_t B, int64_t n_heads, int64_t n_kv_heads,
                              int64_t head_dim, int64_t max_seq, float scale, float softcap, const float* alibi_slopes,
                              void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = q, a.k_cache = k_cache, a.v_cache = v_cache, a.out = out, a.len_dev = len_rows, a.rows = true, a.seq_len = 1, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.softcap = softcap, a.alibi = alibi_slopes;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, false, false);
}

int awq_decode_attention_rope_rows(const uint16_t* qkv, uint16_t* k_cache, uint16_t* v_cache, const float* cos_table,
                                   const float* sin_table, uint16_t* out, const int32_t* pos_rows, int64_t max_len, int64_t B,
                                   int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t max_seq, float scale,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = qkv, a.k_cache = k_cache, a.v_cache = v_cache, a.out = out, a.len_dev = pos_rows, a.rows = true, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.cos_t = cos_table, a.sin_t = sin_table;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, false, true);
}

int awq_decode_attention_ex_fp8(const uint16_t* q, const uint8_t* k_cache, const uint8_t* v_cache, const float* k_scale,
                                const float* v_scale, uint16_t* out, const int32_t* len_dev, int64_t seq_len, int64_t max_len,
                                int64_t B, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t max_seq, float scale,
                                float softcap, const float* alibi_slopes, void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = q, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale, a.out = out;
    a.len_dev = len_dev, a.seq_len = seq_len, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.softcap = softcap, a.alibi = alibi_slopes;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, true, false);
}

int awq_decode_attention_fp8(const uint16_t* q, const uint8_t* k_cache, const uint8_t* v_cache, const float* k_scale,
                             const float* v_scale, uint16_t* out, const int32_t* len_dev, int64_t seq_len, int64_t max_len, int64_t B,
                             int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t max_seq, float scale, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return awq_decode_attention_ex_fp8(q, k_cache, v_cache, k_scale, v_scale, out, len_dev, seq_len, max_len, B, n_heads,
                                       n_kv_heads, head_dim, max_seq, scale, 0.f, nullptr, workspace, workspace_bytes, stream);
}

int awq_decode_attention_rope_fp8(const uint16_t* qkv, uint8_t* k_cache, uint8_t* v_cache, float* k_scale, float* v_scale,
                                  const float* cos_table, const float* sin_table, uint16_t* out, const int32_t* pos_dev,
                                  int64_t start_pos, int64_t max_len, int64_t B, int64_t n_heads, int64_t n_kv_heads,
                                  int64_t head_dim, int64_t max_seq, float scale, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    AwqAttnArgs a;
    a.q = qkv, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale, a.out = out;
    a.len_dev = pos_dev, a.seq_len = start_pos, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.cos_t = cos_table, a.sin_t = sin_table;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, true, true);
}

int awq_decode_attention_rows_fp8(const uint16_t* q, const uint8_t* k_cache, const uint8_t* v_cache, const float* k_scale,
                                  const float* v_scale, uint16_t* out, const int32_t* len_rows, int64_t max_len, int64_t B,
                                  int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t max_seq, float scale, float softcap,
                                  const float* alibi_slopes, void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = q, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale, a.out = out;
    a.len_dev = len_rows, a.rows = true, a.seq_len = 1, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.softcap = softcap, a.alibi = alibi_slopes;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, true, false);
}

int awq_decode_attention_rope_rows_fp8(const uint16_t* qkv, uint8_t* k_cache, uint8_t* v_cache, float* k_scale, float* v_scale,
                                       const float* cos_table, const float* sin_table, uint16_t* out, const int32_t* pos_rows,
                                       int64_t max_len, int64_t B, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                                       int64_t max_seq, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    AwqAttnArgs a;
    a.q = qkv, a.k_cache = k_cache, a.v_cache = v_cache, a.k_scale = k_scale, a.v_scale = v_scale, a.out = out;
    a.len_dev = pos_rows, a.rows = true, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq;
    a.scale = scale, a.cos_t = cos_table, a.sin_t = sin_table;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return decode_attention(a, true, true);
}

// ---- speculative decoding (verify_attn.hip): T new tokens per sequence at per-row device positions
size_t awq_verify_attention_workspace_bytes(int64_t B, int64_t T, int64_t n_heads) {
    if (B <= 0 || T <= 0 || n_heads <= 0 || B * T * n_heads > INT32_MAX / 64) return 0;
    return awq_verify_attention_workspace_bytes_impl((int)B, (int)T, (int)n_heads, 64);
}

int awq_verify_attention_splits(int64_t max_len, int64_t B, int64_t T, int64_t n_heads, int64_t n_kv_heads) {
    if (max_len < 1 || max_len > INT32_MAX || B < 1 || B > 65535 || T < 2 || T > 8 || n_heads < 1 || n_kv_heads < 1 ||
        n_kv_heads > 65535 || n_heads % n_kv_heads)
        return AWQ_ERR_BAD_SHAPE;
    return awq_verify_attention_splits_impl((int)max_len, (int)B, (int)T, (int)n_heads, (int)n_kv_heads);
}

int awq_verify_attention_rows(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, uint16_t* out,
                              const int32_t* pos_rows, int64_t max_len, int64_t B, int64_t T, int64_t n_heads, int64_t n_kv_heads,
                              int64_t head_dim, int64_t max_seq, float scale, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (B < 0 || B > 65535 || n_heads < 1 || n_heads > 65535 || n_kv_heads < 1 || n_kv_heads > 65535 || max_seq < 1 ||
        max_seq > INT32_MAX || max_len < 0 || max_len > INT32_MAX)
        return AWQ_ERR_BAD_SHAPE;
    if (T < 2 || T > 8) return AWQ_ERR_UNSUPPORTED;
    if (B == 0) return AWQ_OK;
    if (!q || !k_cache || !v_cache || !out || !pos_rows) return AWQ_ERR_NULL;
    if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out)) return AWQ_ERR_BAD_ALIGNMENT;
    AwqAttnArgs a;
    a.q = q, a.k_cache = k_cache, a.v_cache = v_cache, a.out = out, a.len_dev = pos_rows, a.rows = true, a.max_len = max_len;
    a.B = B, a.Hq = n_heads, a.Hkv = n_kv_heads, a.D = head_dim, a.Tmax = max_seq, a.scale = scale;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.stream = static_cast<hipStream_t>(stream);
    return awq_launch_verify_attention(a, (int)T);
}

// ---- fp8 KV cache (decoder.hip, KV8): fp16 rows <-> codes + scales
int awq_kv_quant_fp8(const uint16_t* x, uint8_t* cache, float* scales, int64_t B, int64_t S, int64_t n_kv_heads, int64_t head_dim,
                     int64_t max_seq, int64_t start_pos, void* stream) {
    if (B < 0 || S < 0 || n_kv_heads < 1 || max_seq < 1 || max_seq > INT32_MAX || start_pos < 0 || start_pos + S > max_seq ||
        B * max_seq * n_kv_heads > INT32_MAX * (int64_t)16)
        return AWQ_ERR_BAD_SHAPE;
    if (B * S == 0) return AWQ_OK;
    if (!x) return AWQ_ERR_NULL;
    if (int rc = kv8_check(cache, cache, scales, scales, head_dim)) return rc;
    if (!aligned16(x)) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_kv_quant_fp8(x, cache, scales, (int)B, (int)S, (int)n_kv_heads, (int)max_seq, (int)start_pos,
                                   static_cast<hipStream_t>(stream));
}

int awq_kv_dequant_fp8(const uint8_t* cache, const float* scales, uint16_t* out, int64_t B, int64_t n, int64_t n_kv_heads,
                       int64_t head_dim, int64_t max_seq, void* stream) {
    if (B < 0 || n < 0 || n_kv_heads < 1 || max_seq < 1 || max_seq > INT32_MAX || n > max_seq ||
        B * max_seq * n_kv_heads > INT32_MAX * (int64_t)16)
        return AWQ_ERR_BAD_SHAPE;
    if (B * n == 0) return AWQ_OK;
    if (!out) return AWQ_ERR_NULL;
    if (int rc = kv8_check(cache, cache, scales, scales, head_dim)) return rc;
    if (!aligned16(out)) return AWQ_ERR_BAD_ALIGNMENT;
    return awq_launch_kv_dequant_fp8(cache, scales, out, (int)B, (int)n, (int)n_kv_heads, (int)max_seq,
                                     static_cast<hipStream_t>(stream));
}

// ---- token log-probabilities (logprob.hip): every refusal before the launch
int awq_token_logprobs(const AwqLogprobArgs* a) {
    if (!a) return AWQ_ERR_NULL;
    if (a->V < 1 || a->V > ((int64_t)1 << 20) || a->R < 0 || a->R > INT32_MAX || a->logits_stride < a->V) return AWQ_ERR_BAD_SHAPE;
    if (a->R == 0) return AWQ_OK;
    if (!a->logits || !a->ids || !a->out) return AWQ_ERR_NULL;
    return awq_launch_token_logprobs(*a);
}
