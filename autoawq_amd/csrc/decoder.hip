// decoder.hip -- the small kernels around the int4 Linears of a fused decoder block
// (SURVEY.md 8f rank 2): RMSNorm (+ residual add), RoPE + KV-cache append, single-query attention
// over the cache.  All HBM-bound byte movers; fp32 arithmetic, one rounding to fp16.
//
// What they replace in the reference (under /root/reference):
//   awq_rmsnorm         awq_ext.layernorm_forward_cuda(x, weight, out, eps)   awq/modules/fused/norm.py:33-36
//   awq_add_rmsnorm     `h = hidden_states + attn_output` + the next norm     awq/modules/fused/block.py:108-119
//   awq_rope_kv_append  RoPE.forward + WindowedCache.update_kv                awq/modules/fused/attn.py:54-87,265-276, cache.py:40-45
//   awq_decode_attention  flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens, causal=True)  attn.py:291-302
// (awq_ext / flash-attn sources are not in the reference tree: semantics from the call sites and
// from the torch code around them.)
#include <type_traits>

#include "awq_device.h"
#include "awq_internal.h"

namespace {

// Cross-lane moves INSIDE a 16-lane row as DPP operands (a few cycles) instead of __shfl_xor (ds_bpermute: an LDS-crossbar round
// trip of ~100 cycles each, and the attention inner loop made four of them per score, dependent on each other).
template <int CTRL>
AWQ_DEV float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// sum over the 16 lanes of a row, in every lane: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:4, row_ror:8
#ifndef AWQ_ATTN_NO_DPP
#define AWQ_ATTN_NO_DPP 0  // experiment builds: 1 = the __shfl_xor butterflies of rounds 1-3
#endif
// (dpp: uniform.  A/B on the whole decoder, profiles/r04_attention_split_ab.txt: the DPP form gains 1.5-3 % in single-split launches --
// short contexts, where the kernel is a latency chain on 32 blocks -- and LOSES 6-10 % at 2048 tokens of context, where the
// launch is memory-bound and the faster consumption only puts more requests in flight; so the launch shape picks the form.)
AWQ_DEV float row16_sum(float s, bool dpp) {
    if (AWQ_ATTN_NO_DPP || !dpp) {
#pragma unroll
        for (int x = 8; x > 0; x >>= 1) s += __shfl_xor(s, x, 64);
        return s;
    }
    s += dpp_f<0xB1>(s);
    s += dpp_f<0x4E>(s);
    s += dpp_f<0x124>(s);
    s += dpp_f<0x128>(s);
    return s;
}

AWQ_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------- fp8 KV rows (format: include/awq_hip.h, "fp8 KV cache")
// A 128-value row is held 16 lanes x 8 values (lane c: dims 8c .. 8c+7), as the attention kernel reads it.
// max over the 16 lanes of a row, same DPP moves as row16_sum; v >= 0 (|x| bit patterns of fp16: NaN > inf > every finite value,
// so an integer max keeps a NaN that fmaxf would drop)
AWQ_DEV int row16_max_i(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false));
    return v;
}

// codes (8 bytes) of this lane's 8 values and, in every lane of the row, the row's scale 2^k: k the smallest integer with
// amax <= 448 * 2^k, taken from the exponent and mantissa bits of amax (448 = 1.75 * 2^8).  Zero row: scale 0, codes 0.
// A NaN / inf anywhere in the row: scale NaN (every read of the row is then NaN), codes 0.
AWQ_DEV u32x2 kv8_quant_row(const half8_t& h, float& scale) {
    const u32x4 bits = __builtin_bit_cast(u32x4, h);
    int amax = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) amax = max(amax, (int)max(bits[e] & 0x7FFFu, (bits[e] >> 16) & 0x7FFFu));
    amax = row16_max_i(amax);
    u32x2 w = {0u, 0u};
    if (amax >= 0x7C00) {
        scale = __builtin_nanf("");
        return w;
    }
    if (amax == 0) {
        scale = 0.f;
        return w;
    }
    const uint32_t u = __builtin_bit_cast(uint32_t, (float)__builtin_bit_cast(half_t, (uint16_t)amax));  // fp32-normal: >= 2^-24
    const int k = (int)(u >> 23) - 127 - 8 + ((u & 0x7FFFFF) > 0x600000 ? 1 : 0);                       // -32 .. 8
    scale = __builtin_bit_cast(float, (uint32_t)(127 + k) << 23);
    const float inv = __builtin_bit_cast(float, (uint32_t)(127 - k) << 23);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = fminf(fmaxf((float)h[e] * inv, -448.f), 448.f);  // exact scaling; the clamp is a guard
    w.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
    w.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], (int)w.x, true);
    w.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0, false);
    w.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], (int)w.y, true);
    return w;
}

// the 8 codes of a lane as fp32 (exact; the row's scale is applied by the caller)
AWQ_DEV void kv8_decode8(u32x2 w, float* f) {
    auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false);
    auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
    auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false);
    auto d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
    f[0] = a[0], f[1] = a[1], f[2] = b[0], f[3] = b[1], f[4] = c[0], f[5] = c[1], f[6] = d[0], f[7] = d[1];
}

// The attention kernel's cache arguments: a pointer to fp16 rows, or (KV8) the codes and the scales of one cache.
struct KV8Rows {
    uint8_t* codes;
    float* scales;
};
template <bool KV8>
using kv_rows_t = std::conditional_t<KV8, KV8Rows, half_t* __restrict__>;
struct KV8New {  // the new token of the fused form, quantized
    u32x2 k, v;
    float ks, vs;
};
struct KV8None {};

// the fp16 row of an fp8 append before it is quantized
AWQ_DEV half_t* kv8_rowbuf() {
    __shared__ alignas(16) half_t buf[128];  // read back as half8_t
    return buf;
}

template <bool KV8, class RowT>
AWQ_DEV float kv_elem(const RowT& raw, const float* dec, int e) {
    if constexpr (KV8) return dec[e];
    else return (float)raw[e];
}

// ---------------------------------------------------------------- RMSNorm (+ residual add)
// One 256-thread block per row; thread t owns 16-byte chunks t, t+256, ... (H % 8 == 0).
// y = fp16( x * rsqrt(mean(x^2) + eps) * w ), all in fp32, one rounding.
// ADD: r = fp16(residual + x) is written back to `residual` first and is what gets normalised
// (the fp16 rounding of the sum is what torch's `h = hidden_states + attn_output` hands the norm).
template <bool ADD>
__global__ __launch_bounds__(256) void awq_rmsnorm_kernel(const half_t* __restrict__ x, half_t* __restrict__ residual,
                                                         const half_t* __restrict__ w, half_t* __restrict__ out, int H,
                                                         float eps) {
    constexpr int MAXC = 8;  // chunks per thread kept in registers: H <= 16384
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int chunks = H >> 3;
    half8_t v[MAXC];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = tid + 256 * i;
        if (c < chunks) {
            v[i] = *reinterpret_cast<const half8_t*>(x + (int64_t)row * H + 8 * c);
            if constexpr (ADD) {
                const half8_t r = *reinterpret_cast<const half8_t*>(residual + (int64_t)row * H + 8 * c);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = (half_t)((float)v[i][e] + (float)r[e]);
                *reinterpret_cast<half8_t*>(residual + (int64_t)row * H + 8 * c) = v[i];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += (float)v[i][e] * (float)v[i][e];
        }
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float inv = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)H + eps);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = tid + 256 * i;
        if (c < chunks) {
            const half8_t g = *reinterpret_cast<const half8_t*>(w + 8 * c);
            half8_t o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)v[i][e] * inv * (float)g[e]);
            *reinterpret_cast<half8_t*>(out + (int64_t)row * H + 8 * c) = o;
        }
    }
}

// ---------------------------------------------------------------- RoPE + KV append
// qkv [tokens = B*S, (Hq + 2*Hkv) * D] fp16 as the fused qkv Linear writes it (q heads | k heads |
// v heads).  One block per (token, head slot), D/2 threads; thread i rotates the pair
// (i, i + rot/2) of a q or k head by the angle of position start + s (cos/sin tables
// [max_pos, rot/2] fp32, built like RoPE.precompute_freqs_cis), passes dims >= rot through, and
// writes q to q_out [B*S, Hq, D], k / v to the caches [B, Tmax, Hkv, D] at row start + s.
// ROWS (awq_rope_kv_append_rows): every sequence b has its own start, pos_dev[b] ([B] int32 on the device, never NULL) --
// batches of prompts of different lengths (modules/fused/decode.py); clamped to [0, Tmax - 1] like the shared one.
// COUNTS (awq_rope_kv_append_rows_n*): ROWS with count_dev[b] new tokens in sequence b -- the blocks of slots s >= count_dev[b] leave
// without writing anything (the clamp above would otherwise put a pad slot of a sequence that ends at Tmax on its last real row).
// KV8 (awq_rope_kv_append*_fp8, D = 128: one wave): a k / v block computes its fp16 row exactly as above into LDS, then lanes
// (r, c) quantize it 16 lanes x 8 values (kv8_quant_row) and row 0 writes the 128 codes and the scale.
template <bool ROWS, bool KV8, bool COUNTS = false, class CacheT>
AWQ_DEV void rope_kv_append_body(const half_t* qkv, half_t* q_out, CacheT* k_cache,
                                 CacheT* v_cache, const float* cos_t, const float* sin_t,
                                 const int* pos_dev, int start_pos, int S, int Hq, int Hkv, int D, int rot, int Tmax,
                                 float* k_scale, float* v_scale, const int* count_dev = nullptr) {
    const int slot = blockIdx.x % (Hq + 2 * Hkv), tok = blockIdx.x / (Hq + 2 * Hkv);
    const int b = tok / S, s = tok % S;
    if constexpr (COUNTS) {
        if (s >= count_dev[b]) return;  // (block-uniform)
    }
    // A device-side position (hipGraph replay) is not seen by the host checks: clamp it to the cache so that a
    // replay past max_seq_len overwrites the last row instead of memory behind the cache / the cos-sin tables
    // (the caller is expected to roll the window before that: modules/fused/model.py).
    const int pos = ROWS ? max(0, min(pos_dev[b] + s, Tmax - 1)) : min((pos_dev ? *pos_dev : start_pos) + s, Tmax - 1);
    const int i = threadIdx.x;  // 0 .. D/2-1
    const half_t* src = qkv + (int64_t)tok * (Hq + 2 * Hkv) * D + (int64_t)slot * D;
    half_t* dst;
    if (slot < Hq) dst = q_out + ((int64_t)tok * Hq + slot) * D;
    else if constexpr (KV8) dst = kv8_rowbuf();
    else if (slot < Hq + Hkv) dst = k_cache + (((int64_t)b * Tmax + pos) * Hkv + (slot - Hq)) * D;
    else dst = v_cache + (((int64_t)b * Tmax + pos) * Hkv + (slot - Hq - Hkv)) * D;
    const int half_rot = rot >> 1;
    if (slot < Hq + Hkv && i < half_rot) {
        const float c = cos_t[(int64_t)pos * half_rot + i], sn = sin_t[(int64_t)pos * half_rot + i];
        const float a = (float)src[i], bb = (float)src[i + half_rot];
        dst[i] = (half_t)awq_rope_term(a, bb, c, -sn);
        dst[i + half_rot] = (half_t)awq_rope_term(bb, a, c, sn);
    } else if (slot < Hq + Hkv) {  // pass-through part of a partially rotated head: dims rot .. D-1
        const int d0 = rot + 2 * (i - half_rot);
        if (d0 < D) dst[d0] = src[d0];
        if (d0 + 1 < D) dst[d0 + 1] = src[d0 + 1];
    } else {
        dst[2 * i] = src[2 * i];
        dst[2 * i + 1] = src[2 * i + 1];
    }
    if constexpr (KV8) {
        if (slot >= Hq) {  // (block-uniform)
            __syncthreads();
            const int c = threadIdx.x & 15;
            float sc;
            const u32x2 w = kv8_quant_row(*reinterpret_cast<const half8_t*>(dst + 8 * c), sc);
            const bool is_k = slot < Hq + Hkv;
            const int64_t row = ((int64_t)b * Tmax + pos) * Hkv + (is_k ? slot - Hq : slot - Hq - Hkv);
            if (threadIdx.x < 16) *reinterpret_cast<u32x2*>((is_k ? k_cache : v_cache) + row * 128 + 8 * c) = w;
            if (threadIdx.x == 0) (is_k ? k_scale : v_scale)[row] = sc;
        }
    }
}

template <bool ROWS = false>
__global__ __launch_bounds__(128) void awq_rope_kv_append_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ q_out,
                                                                half_t* __restrict__ k_cache, half_t* __restrict__ v_cache,
                                                                const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                const int* __restrict__ pos_dev, int start_pos, int S, int Hq,
                                                                int Hkv, int D, int rot, int Tmax) {
    rope_kv_append_body<ROWS, false>(qkv, q_out, k_cache, v_cache, cos_t, sin_t, pos_dev, start_pos, S, Hq, Hkv, D, rot, Tmax,
                                     nullptr, nullptr);
}

template <bool ROWS>
__global__ __launch_bounds__(64) void awq_rope_kv_append_fp8_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ q_out,
                                                                   uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
                                                                   float* __restrict__ k_scale, float* __restrict__ v_scale,
                                                                   const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                   const int* __restrict__ pos_dev, int start_pos, int S, int Hq,
                                                                   int Hkv, int rot, int Tmax) {
    rope_kv_append_body<ROWS, true>(qkv, q_out, k_cache, v_cache, cos_t, sin_t, pos_dev, start_pos, S, Hq, Hkv, 128, rot, Tmax,
                                    k_scale, v_scale);
}

__global__ __launch_bounds__(128) void awq_rope_kv_append_n_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ q_out,
                                                                  half_t* __restrict__ k_cache, half_t* __restrict__ v_cache,
                                                                  const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                  const int* __restrict__ pos_dev, const int* __restrict__ count_dev,
                                                                  int S, int Hq, int Hkv, int D, int rot, int Tmax) {
    rope_kv_append_body<true, false, true>(qkv, q_out, k_cache, v_cache, cos_t, sin_t, pos_dev, 0, S, Hq, Hkv, D, rot, Tmax, nullptr,
                                           nullptr, count_dev);
}

__global__ __launch_bounds__(64) void awq_rope_kv_append_n_fp8_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ q_out,
                                                                     uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
                                                                     float* __restrict__ k_scale, float* __restrict__ v_scale,
                                                                     const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                     const int* __restrict__ pos_dev, const int* __restrict__ count_dev,
                                                                     int S, int Hq, int Hkv, int rot, int Tmax) {
    rope_kv_append_body<true, true, true>(qkv, q_out, k_cache, v_cache, cos_t, sin_t, pos_dev, 0, S, Hq, Hkv, 128, rot, Tmax, k_scale,
                                          v_scale, count_dev);
}

// ---------------------------------------------------------------- single-query attention over the cache
// grid (splits, Hkv, B), 256 threads.  A block owns one KV head, the G = Hq/Hkv query heads that
// share it and a contiguous chunk of the sequence.  Lane (r = lane >> 4, c = lane & 15) reads the
// 16 bytes [8c, 8c+8) of cache row t0 + 4*(wave + 4*i) + r: a wave instruction covers four whole
// 256-byte rows (D = 128).  (Round 4 tried HEAD-major caches [B, Hkv, Tmax, D] -- four consecutive rows of a head = 1 KiB of contiguous
// memory per instruction, on the theory that the 2.1 TB/s this kernel reaches at 2048 tokens is the rate of scattered 256-byte
// pieces: no gain at 64 / 512 tokens, -1.5 % at 2048 and -6 % at 200 (one block then reads 50 KB from one region); reverted,
// profiles/r04_attention_split_ab.txt.  The kernel is bound by its per-block latency chain, not by the access granularity.)  Scores by 16-lane butterfly, online softmax per lane group, P*V into
// 8 fp32 accumulators per query head; lane groups, waves and finally the splits are merged with
// the usual (max, sum, acc) rule.  Partial results of a split go to `part` [B, Hq, splits, D + 2]
// fp32 and a second tiny kernel finishes; with one split the block writes fp16 directly.
// FUSED (awq_decode_attention_rope): `q` is the raw fused-qkv row [B, (Hq + 2 Hkv) * D]; the kernel
// rotates its query heads itself (partner dims d +- 64 live in lane c ^ 8), takes the NEW token's
// rotated k and its v straight from that row -- cache row `pos` is not read by anybody in this
// launch -- and the one block whose chunk holds `pos` appends them to the caches.  len_dev then
// holds the POSITION (length - 1).  Same roundings as awq_rope_kv_append followed by the plain
// kernel: one rotation for both (awq_rope_term, awq_device.h), rotated values pass through fp16.
// EXTRA (plain form only): logit soft-capping s := cap * tanh(s / cap) (attn.py:150,166 `softcap=`) and ALiBi, a per-head linear
// bias slope_h * (t - pos) on the key position (attn.py:89-125,149,165 `alibi_slopes=`), in that order like flash-attn.
// ROWS (the *_rows entry points): len_dev is [B], sequence b reads its own length (FUSED: position) from len_dev[b].  The launch
// is still sized on the host for the bucket's bound; a block deals the rows of ITS sequence to the splits, so a short sequence in
// a long bucket leaves the last splits empty -- they write the (-inf, 0) partial the combine kernel gives weight 0.
// KV8 (the *_fp8 entry points): kc / vc are KV8Rows, the caches hold e4m3 codes, one byte per value, and their `scales` one
// fp32 scale per (sequence, row, KV head).  Same geometry: lane (r, c) loads the 8 bytes [8c, 8c+8) of its row, and the row's two
// scales in the same round trip; the score is scale_k * sum q*code, the V weight p * scale_v.  FUSED quantizes the new token's
// k / v (kv8_quant_row) and uses the quantized values for its own score and value, as append + plain would.
template <int G, bool FUSED, bool EXTRA = false, bool ROWS = false, bool KV8 = false>
__global__ __launch_bounds__(256) void awq_decode_attn_kernel(const half_t* __restrict__ q, kv_rows_t<KV8> kc,
                                                             kv_rows_t<KV8> vc, half_t* __restrict__ out,
                                                             float* __restrict__ part, const int* __restrict__ len_dev,
                                                             int seq_len, int Hq, int Hkv, int Tmax, float scale,
                                                             int chunk, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, float softcap,
                                                             const float* __restrict__ alibi) {
    using CacheT = std::conditional_t<KV8, uint8_t, half_t>;
    using RowT = std::conditional_t<KV8, u32x2, half8_t>;
    static_assert(!(FUSED && EXTRA), "soft-capping / ALiBi ride on the plain form");
    constexpr int D = 128;
    __shared__ float sm[4][G][D + 2];
    const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane >> 4, c = lane & 15;
    // A launch with ONE split starts at row 0 whatever the length is: its first row sets are requested HERE, before the length,
    // the rotation tables and the query have made their own round trips (at 64 tokens of context the kernel is nothing but a chain
    // of dependent round trips on 32 blocks; rows at or past the length are requested too -- they exist, the cache is Tmax rows --
    // and never used: `live` below).  Later row sets and launches with several splits request inside the loop as before.
    constexpr int U = 4;  // row sets requested before any is consumed: 8 loads of 16 bytes in flight per lane
    const int64_t rowstride = (int64_t)Hkv * D;
    const CacheT* kb;
    const CacheT* vb;
    const float* ksb = nullptr;  // KV8: row t's scale at ksb[t * Hkv]
    const float* vsb = nullptr;
    if constexpr (KV8) {
        kb = kc.codes + ((int64_t)b * Tmax * Hkv + hk) * D + 8 * c;
        vb = vc.codes + ((int64_t)b * Tmax * Hkv + hk) * D + 8 * c;
        ksb = kc.scales + (int64_t)b * Tmax * Hkv + hk;
        vsb = vc.scales + (int64_t)b * Tmax * Hkv + hk;
    } else {
        kb = kc + ((int64_t)b * Tmax * Hkv + hk) * D + 8 * c;
        vb = vc + ((int64_t)b * Tmax * Hkv + hk) * D + 8 * c;
    }
#ifndef AWQ_ATTN_NO_EARLY
#define AWQ_ATTN_NO_EARLY 0  // experiment builds: 1 = request every row set inside the loop (round 3's order)
#endif
    const bool early = gridDim.x == 1 && !AWQ_ATTN_NO_EARLY;
    RowT kv0[U], vv0[U];
    float ks0[U], vs0[U];  // KV8: the rows' scales
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = 4 * wave + 16 * u + r;
        kv0[u] = RowT{};
        vv0[u] = kv0[u];
        ks0[u] = vs0[u] = 0.f;
        if (early && t < Tmax) {
            kv0[u] = *reinterpret_cast<const RowT*>(kb + (int64_t)t * rowstride);
            vv0[u] = *reinterpret_cast<const RowT*>(vb + (int64_t)t * rowstride);
            if constexpr (KV8) {
                ks0[u] = ksb[(int64_t)t * Hkv];
                vs0[u] = vsb[(int64_t)t * Hkv];
            }
        }
    }
    // device-side lengths are clamped to the cache (see awq_rope_kv_append_kernel): never a row >= Tmax
    const int T = max(1, min((ROWS ? len_dev[b] : (len_dev ? *len_dev : seq_len)) + (FUSED ? 1 : 0), Tmax));
    const int pos = T - 1;  // FUSED: the new token's position
    // The rows are dealt to the splits of the launch HERE, from the length the device knows (round 4): a launch sized on the host
    // for a longer context (a hipGraph serves every length up to its bucket's bound) still spreads the rows that exist over
    // all of its splits instead of leaving them to the first few.  16-row granularity (a wave instruction covers 4 rows).
    if (chunk <= 0) chunk = (((T + (int)gridDim.x - 1) / (int)gridDim.x) + 15) & ~15;
    const int t0 = split * chunk, t1 = min(T, t0 + chunk);

    float qf[G][8];
    half8_t k_new = {0, 0, 0, 0, 0, 0, 0, 0}, v_new = k_new;
    std::conditional_t<KV8, KV8New, KV8None> nq{};  // KV8: the new token's codes and scales
    if constexpr (FUSED) {
        const half_t* row = q + (int64_t)b * (Hq + 2 * Hkv) * D;
        float cs[8], sn[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = (8 * c + e) & 63;
            cs[e] = cos_t[(int64_t)pos * 64 + i];
            sn[e] = sin_t[(int64_t)pos * 64 + i];
            if (c < 8) sn[e] = -sn[e];  // lanes c < 8 hold dims d < 64: a c - b s; the others b c + a s (awq_rope_term)
        }
        auto rotate = [&](half8_t x) -> half8_t {
            half8_t o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float mine = (float)x[e], other = AWQ_ATTN_NO_DPP ? __shfl_xor(mine, 8, 64) : dpp_f<0x128>(mine);  // row_ror:8 = lane c ^ 8 of the row: dims d and d +- 64
                o[e] = (half_t)awq_rope_term(mine, other, cs[e], sn[e]);
            }
            return o;
        };
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const half8_t qr = rotate(*reinterpret_cast<const half8_t*>(row + (int64_t)(hk * G + g) * D + 8 * c));
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[g][e] = (float)qr[e] * scale;
        }
        k_new = rotate(*reinterpret_cast<const half8_t*>(row + (int64_t)(Hq + hk) * D + 8 * c));
        v_new = *reinterpret_cast<const half8_t*>(row + (int64_t)(Hq + Hkv + hk) * D + 8 * c);
        if constexpr (KV8) {
            nq.k = kv8_quant_row(k_new, nq.ks);
            nq.v = kv8_quant_row(v_new, nq.vs);
            if (pos >= t0 && pos < t1 && wave == 0 && r == 0) {  // append: one block, 16 lanes x 8 bytes per cache + the scales
                const int64_t row = ((int64_t)b * Tmax + pos) * Hkv + hk;
                *reinterpret_cast<u32x2*>(kc.codes + row * D + 8 * c) = nq.k;
                *reinterpret_cast<u32x2*>(vc.codes + row * D + 8 * c) = nq.v;
                if (c == 0) {
                    kc.scales[row] = nq.ks;
                    vc.scales[row] = nq.vs;
                }
            }
        } else if (pos >= t0 && pos < t1 && wave == 0 && r == 0) {  // append: one block, 16 lanes x 16 bytes per cache
            *reinterpret_cast<half8_t*>(kc + (((int64_t)b * Tmax + pos) * Hkv + hk) * D + 8 * c) = k_new;
            *reinterpret_cast<half8_t*>(vc + (((int64_t)b * Tmax + pos) * Hkv + hk) * D + 8 * c) = v_new;
        }
    } else {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const half8_t qv = *reinterpret_cast<const half8_t*>(q + ((int64_t)b * Hq + hk * G + g) * D + 8 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[g][e] = (float)qv[e] * scale;
        }
    }
    float slope[G];
#pragma unroll
    for (int g = 0; g < G; ++g) slope[g] = (EXTRA && alibi) ? alibi[hk * G + g] : 0.f;
    const float inv_cap = (EXTRA && softcap > 0.f) ? 1.0f / softcap : 0.f;
    float m[G], l[G], o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY;
        l[g] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
    }
    for (int tb = t0 + 4 * wave; tb < t1; tb += 16 * U) {  // wave-uniform trip count
        RowT kv[U], vv[U];
        float ks[U], vs[U];
        const bool first = early && tb == 4 * wave;  // (uniform) these row sets were requested at the top of the kernel
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = tb + 16 * u + r;
            kv[u] = kv0[u];
            vv[u] = vv0[u];
            ks[u] = ks0[u];
            vs[u] = vs0[u];
            if (!first) {
                kv[u] = RowT{};
                vv[u] = kv[u];
                ks[u] = vs[u] = 0.f;
                if (t < t1 && !(FUSED && t == pos)) {
                    kv[u] = *reinterpret_cast<const RowT*>(kb + (int64_t)t * rowstride);
                    vv[u] = *reinterpret_cast<const RowT*>(vb + (int64_t)t * rowstride);
                    if constexpr (KV8) {
                        ks[u] = ksb[(int64_t)t * Hkv];
                        vs[u] = vsb[(int64_t)t * Hkv];
                    }
                }
            }
            if constexpr (KV8) {
                if (FUSED && t == pos) {  // the new token, quantized
                    kv[u] = nq.k;
                    vv[u] = nq.v;
                    ks[u] = nq.ks;
                    vs[u] = nq.vs;
                }
            } else if (FUSED && t == pos) {  // the new token: from the qkv row, not from the cache
                kv[u] = k_new;
                vv[u] = v_new;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = tb + 16 * u + r < t1;
            float kd[8], vd[8];  // KV8: the codes as fp32
            if constexpr (KV8) {
                kv8_decode8(kv[u], kd);
                kv8_decode8(vv[u], vd);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) s += qf[g][e] * kv_elem<KV8>(kv[u], kd, e);
                s = row16_sum(s, early);  // sum over the 16 lanes of the row
                if constexpr (KV8) s *= ks[u];
                if constexpr (EXTRA) {
                    if (inv_cap > 0.f) s = softcap * tanhf(s * inv_cap);
                    s += slope[g] * (float)(tb + 16 * u + r - pos);
                }
                if (live) {
                    const float mn = fmaxf(m[g], s);
                    const float corr = __expf(m[g] - mn), p = __expf(s - mn);
                    l[g] = l[g] * corr + p;
                    const float pv = KV8 ? p * vs[u] : p;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[g][e] = o[g][e] * corr + pv * kv_elem<KV8>(vv[u], vd, e);
                    m[g] = mn;
                }
            }
        }
    }
    // merge the four lane groups of the wave (lanes c, c+16, c+32, c+48 hold the same dims)
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
            const float mo = __shfl_xor(m[g], x, 64), lo = __shfl_xor(l[g], x, 64);
            const float mn = fmaxf(m[g], mo);
            const float ca = (m[g] == -INFINITY) ? 0.f : __expf(m[g] - mn), cb = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[g][e] = o[g][e] * ca + __shfl_xor(o[g][e], x, 64) * cb;
            l[g] = l[g] * ca + lo * cb;
            m[g] = mn;
        }
        if (r == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[wave][g][8 * c + e] = o[g][e];
            if (c == 0) {
                sm[wave][g][D] = m[g];
                sm[wave][g][D + 1] = l[g];
            }
        }
    }
    __syncthreads();
    // merge the four waves: thread (g, d) for g < G, d < 128 -> G*128 threads (G <= 2) or a loop
    const int nsplit = gridDim.x;
    for (int idx = tid; idx < G * D; idx += 256) {
        const int g = idx / D, d = idx % D;
        float mn = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mn = fmaxf(mn, sm[w][g][D]);
        float acc = 0.f, ls = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float cw = (sm[w][g][D] == -INFINITY) ? 0.f : __expf(sm[w][g][D] - mn);
            acc += sm[w][g][d] * cw;
            ls += sm[w][g][D + 1] * cw;
        }
        if constexpr (KV8) {
            // a NaN scale (a row that held a NaN or an inf) makes the weights NaN, and `ls > 0` below would turn that into 0: keep it
            // NaN, also through the combine kernel (this split then carries all the weight: NaN / inf)
            if (ls != ls) {
                acc = __builtin_nanf("");
                ls = INFINITY;
                mn = 3.402823466e38f;
            }
        }
        const int64_t head = (int64_t)b * Hq + hk * G + g;
        if (nsplit == 1) {
            out[head * D + d] = (half_t)(ls > 0.f ? acc / ls : 0.f);
        } else {
            float* pp = part + (head * nsplit + split) * (D + 2);
            pp[d] = acc;
            if (d == 0) {
                pp[D] = mn;
                pp[D + 1] = ls;
            }
        }
    }
}

// One block per (sequence, query head): lanes of wave 0 take one split each (max, weights, sum by
// wave reductions), then thread d adds the splits' accumulators with independent loads.  (The first
// version walked the splits serially twice: 12 us for 32 splits, more than the attention itself.)
__global__ __launch_bounds__(128) void awq_decode_attn_combine_kernel(const float* __restrict__ part, half_t* __restrict__ out,
                                                                     int nsplit) {
    constexpr int D = 128;
    __shared__ float wgt[64];
    __shared__ float denom;
    const int64_t head = blockIdx.x;
    const int d = threadIdx.x;
    const float* pp = part + head * nsplit * (D + 2);
    if (d < 64) {  // nsplit <= 64
        const float ms = d < nsplit ? pp[d * (D + 2) + D] : -INFINITY;
        const float ls = d < nsplit ? pp[d * (D + 2) + D + 1] : 0.f;
        float mn = ms;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = fmaxf(mn, __shfl_xor(mn, o, 64));
        const float w = (ms == -INFINITY) ? 0.f : __expf(ms - mn);
        wgt[d] = w;
        const float tot = wave_sum(ls * w);
        if (d == 0) denom = tot;
    }
    __syncthreads();
    float acc = 0.f;
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) acc += pp[s * (D + 2) + d] * wgt[s];
    out[head * D + d] = (half_t)(denom > 0.f ? acc / denom : 0.f);
}

// ---------------------------------------------------------------- fp8 cache rows <-> fp16 (prefill workspace, update_kv, tests)
// 16 lanes per (sequence, row, KV head), 8 values each; 256 threads = 16 rows per block.  Row i of the flat [B, n, Hkv] index is
// cache row (b, start + t, h) of a [*, Tmax, Hkv, 128] cache.
// dequant: out [B, n, Hkv, 128] fp16 = fp16(code * scale) for cache rows [0, n), saturated to +-65504 (a NaN scale stays NaN).
__global__ __launch_bounds__(256) void awq_kv_dequant_fp8_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scales,
                                                                 half_t* __restrict__ out, int n, int Hkv, int Tmax, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (i >= rows) return;
    const int64_t per = (int64_t)n * Hkv, src = (i / per) * Tmax * Hkv + i % per;
    const u32x2 w = *reinterpret_cast<const u32x2*>(codes + src * 128 + 8 * c);
    const float sc = scales[src];
    float f[8];
    kv8_decode8(w, f);
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = f[e] * sc;
        o[e] = (half_t)(fabsf(v) > 65504.f ? copysignf(65504.f, v) : v);
    }
    *reinterpret_cast<half8_t*>(out + i * 128 + 8 * c) = o;
}

// quant: x [B, S, Hkv, 128] fp16 -> codes and scales of cache rows [start, start + S)
__global__ __launch_bounds__(256) void awq_kv_quant_fp8_kernel(const half_t* __restrict__ x, uint8_t* __restrict__ codes,
                                                               float* __restrict__ scales, int S, int Hkv, int Tmax, int start,
                                                               int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (i >= rows) return;  // (whole 16-lane rows: the DPP max stays inside live lanes)
    const int64_t per = (int64_t)S * Hkv, dst = (i / per) * Tmax * Hkv + (int64_t)start * Hkv + i % per;
    float sc;
    const u32x2 w = kv8_quant_row(*reinterpret_cast<const half8_t*>(x + i * 128 + 8 * c), sc);
    *reinterpret_cast<u32x2*>(codes + dst * 128 + 8 * c) = w;
    if (c == 0) scales[dst] = sc;
}

}  // namespace

int awq_launch_rmsnorm(const uint16_t* x, uint16_t* residual, const uint16_t* w, uint16_t* out, int64_t M, int64_t H,
                       float eps, hipStream_t st) {
    if (M < 0 || H <= 0 || H % 8 || H > 16384) return AWQ_ERR_BAD_SHAPE;
    if (M == 0) return AWQ_OK;
    if (residual)
        hipLaunchKernelGGL(awq_rmsnorm_kernel<true>, dim3((unsigned)M), dim3(256), 0, st, reinterpret_cast<const half_t*>(x),
                           reinterpret_cast<half_t*>(residual), reinterpret_cast<const half_t*>(w),
                           reinterpret_cast<half_t*>(out), (int)H, eps);
    else
        hipLaunchKernelGGL(awq_rmsnorm_kernel<false>, dim3((unsigned)M), dim3(256), 0, st, reinterpret_cast<const half_t*>(x),
                           nullptr, reinterpret_cast<const half_t*>(w), reinterpret_cast<half_t*>(out), (int)H, eps);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

int awq_launch_rope_kv_append(const AwqAppendArgs& a) {
    const int start_pos = (int)a.start_pos, B = (int)a.B, S = (int)a.S, Hq = (int)a.Hq, Hkv = (int)a.Hkv, D = (int)a.D, rot = (int)a.rot,
              Tmax = (int)a.Tmax;
    if (B < 0 || S < 0 || Hq < 1 || Hkv < 1 || D < 2 || D % 2 || D > 256 || rot < 0 || rot > D || rot % 2)
        return AWQ_ERR_BAD_SHAPE;
    if (a.rows && !a.pos_dev) return AWQ_ERR_NULL;
    if (a.count_dev && !a.rows) return AWQ_ERR_BAD_SHAPE;
    if (!a.pos_dev && (start_pos < 0 || start_pos + S > Tmax)) return AWQ_ERR_BAD_SHAPE;
    const bool kv8 = a.k_scale != nullptr;
    if (kv8 && !a.v_scale) return AWQ_ERR_NULL;
    if (kv8 && D != 128) return AWQ_ERR_UNSUPPORTED;
    if (B * S == 0) return AWQ_OK;
    const unsigned blocks = (unsigned)((int64_t)B * S * (Hq + 2 * Hkv));
    const half_t* qkv = reinterpret_cast<const half_t*>(a.qkv);
    half_t* q_out = reinterpret_cast<half_t*>(a.q_out);
    if (a.count_dev && kv8)
        hipLaunchKernelGGL(awq_rope_kv_append_n_fp8_kernel, dim3(blocks), dim3(64), 0, a.stream, qkv, q_out,
                           static_cast<uint8_t*>(a.k_cache), static_cast<uint8_t*>(a.v_cache), a.k_scale, a.v_scale, a.cos_t, a.sin_t,
                           a.pos_dev, a.count_dev, S, Hq, Hkv, rot, Tmax);
    else if (a.count_dev)
        hipLaunchKernelGGL(awq_rope_kv_append_n_kernel, dim3(blocks), dim3(D / 2), 0, a.stream, qkv, q_out,
                           static_cast<half_t*>(a.k_cache), static_cast<half_t*>(a.v_cache), a.cos_t, a.sin_t, a.pos_dev, a.count_dev, S,
                           Hq, Hkv, D, rot, Tmax);
    else if (kv8)
        hipLaunchKernelGGL(a.rows ? awq_rope_kv_append_fp8_kernel<true> : awq_rope_kv_append_fp8_kernel<false>, dim3(blocks), dim3(64),
                           0, a.stream, qkv, q_out, static_cast<uint8_t*>(a.k_cache), static_cast<uint8_t*>(a.v_cache), a.k_scale,
                           a.v_scale, a.cos_t, a.sin_t, a.pos_dev, start_pos, S, Hq, Hkv, rot, Tmax);
    else
        hipLaunchKernelGGL(a.rows ? awq_rope_kv_append_kernel<true> : awq_rope_kv_append_kernel<false>, dim3(blocks), dim3(D / 2), 0,
                           a.stream, qkv, q_out, static_cast<half_t*>(a.k_cache), static_cast<half_t*>(a.v_cache), a.cos_t, a.sin_t,
                           a.pos_dev, start_pos, S, Hq, Hkv, D, rot, Tmax);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

size_t awq_decode_attention_workspace_bytes_impl(int B, int Hq, int max_splits) {
    return (size_t)B * Hq * max_splits * (128 + 2) * sizeof(float);
}

// The kernel's view of a cache.  The pointers lose their const here: only the fused form writes through them.
template <bool KV8>
static kv_rows_t<KV8> cache_rows(const void* cache, const float* scales) {
    if constexpr (KV8) return KV8Rows{static_cast<uint8_t*>(const_cast<void*>(cache)), const_cast<float*>(scales)};
    else return static_cast<half_t*>(const_cast<void*>(cache));
}

// One launch of awq_decode_attn_kernel<G, FUSED, EXTRA, ROWS, KV8>: the kernel's argument list is written here and nowhere else.
// An fp8 cache (scales given) is a flag of every form.
template <int G, bool FUSED, bool EXTRA, bool ROWS>
static void launch_attn_kernel(const AwqAttnArgs& a, dim3 grid) {
    const int chunk = 0;  // dealt in the kernel from the length it reads
    const auto launch = [&](auto kv8) {
        constexpr bool KV8 = decltype(kv8)::value;
        hipLaunchKernelGGL((awq_decode_attn_kernel<G, FUSED, EXTRA, ROWS, KV8>), grid, dim3(256), 0, a.stream,
                           reinterpret_cast<const half_t*>(a.q), cache_rows<KV8>(a.k_cache, a.k_scale),
                           cache_rows<KV8>(a.v_cache, a.v_scale), reinterpret_cast<half_t*>(a.out), static_cast<float*>(a.workspace),
                           a.len_dev, (int)a.seq_len, (int)a.Hq, (int)a.Hkv, (int)a.Tmax, a.scale, chunk, a.cos_t, a.sin_t,
                           EXTRA ? a.softcap : 0.f, a.alibi);
    };
    if (a.k_scale) launch(std::true_type{});
    else launch(std::false_type{});
}

enum class AttnForm { Plain, Fused, Extra };  // (soft-capping / ALiBi ride on the plain form: there is no fused + extra kernel)

// the form becomes a template flag here; the fp8 cache in launch_attn_kernel
template <int G, bool ROWS>
static void launch_attn(AttnForm form, const AwqAttnArgs& a, dim3 grid) {
    switch (form) {
        case AttnForm::Extra: return launch_attn_kernel<G, false, true, ROWS>(a, grid);
        case AttnForm::Fused: return launch_attn_kernel<G, true, false, ROWS>(a, grid);
        case AttnForm::Plain: return launch_attn_kernel<G, false, false, ROWS>(a, grid);
    }
}

// cos_t == nullptr: plain form (q [B, Hq, D], rows [0, len) of the caches).  Otherwise the fused form:
// q = raw qkv rows, `len_dev` / `seq_len` carry the POSITION of the new token.  rows: len_dev is [B], one word per sequence.
int awq_launch_decode_attention(const AwqAttnArgs& a) {
    const int seq_len = (int)a.seq_len, max_len = (int)a.max_len, B = (int)a.B, Hq = (int)a.Hq, Hkv = (int)a.Hkv, Tmax = (int)a.Tmax;
    if (a.rows && !a.len_dev) return AWQ_ERR_NULL;
    if ((a.k_scale == nullptr) != (a.v_scale == nullptr)) return AWQ_ERR_NULL;
    if ((int)a.D != 128) return AWQ_ERR_UNSUPPORTED;
    const bool extra = a.softcap > 0.f || a.alibi != nullptr, fused = a.cos_t != nullptr;
    if (extra && fused) return AWQ_ERR_UNSUPPORTED;  // ALiBi models do not rotate; soft-capping takes the two-launch form
    if (a.softcap < 0.f) return AWQ_ERR_BAD_SHAPE;
    if (B < 0 || Hq < 1 || Hkv < 1 || Hq % Hkv || Tmax < 1) return AWQ_ERR_BAD_SHAPE;
    const int G = Hq / Hkv;
    if (!(G == 1 || G == 2 || G == 4 || G == 8)) return AWQ_ERR_UNSUPPORTED;
    if (B == 0) return AWQ_OK;
    // the split must not depend on a length that only the device knows: size it for max_len
    const int len_for_split = a.len_dev ? max_len : seq_len + (fused ? 1 : 0);
    if (len_for_split < 1 || len_for_split > Tmax) return AWQ_ERR_BAD_SHAPE;
    const int splits = awq_attn_splits(len_for_split, (int64_t)B * Hkv, a.workspace ? a.workspace_bytes : 0,
                                       awq_decode_attention_workspace_bytes_impl(B, Hq, 1));
    const dim3 grid((unsigned)splits, (unsigned)Hkv, (unsigned)B);
    const AttnForm form = extra ? AttnForm::Extra : fused ? AttnForm::Fused : AttnForm::Plain;
    switch (G) {
        case 1: a.rows ? launch_attn<1, true>(form, a, grid) : launch_attn<1, false>(form, a, grid); break;
        case 2: a.rows ? launch_attn<2, true>(form, a, grid) : launch_attn<2, false>(form, a, grid); break;
        case 4: a.rows ? launch_attn<4, true>(form, a, grid) : launch_attn<4, false>(form, a, grid); break;
        default: a.rows ? launch_attn<8, true>(form, a, grid) : launch_attn<8, false>(form, a, grid);
    }
    if (hipGetLastError() != hipSuccess) return AWQ_ERR_LAUNCH;
    if (splits > 1) {
        hipLaunchKernelGGL(awq_decode_attn_combine_kernel, dim3((unsigned)(B * Hq)), dim3(128), 0, a.stream,
                           static_cast<float*>(a.workspace), reinterpret_cast<half_t*>(a.out), splits);
        if (hipGetLastError() != hipSuccess) return AWQ_ERR_LAUNCH;
    }
    return AWQ_OK;
}

int awq_launch_kv_quant_fp8(const uint16_t* x, uint8_t* codes, float* scales, int B, int S, int Hkv, int Tmax, int start,
                            hipStream_t st) {
    if (B < 0 || S < 0 || Hkv < 1 || start < 0 || start + S > Tmax) return AWQ_ERR_BAD_SHAPE;
    const int64_t rows = (int64_t)B * S * Hkv;
    if (rows == 0) return AWQ_OK;
    hipLaunchKernelGGL(awq_kv_quant_fp8_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st,
                       reinterpret_cast<const half_t*>(x), codes, scales, S, Hkv, Tmax, start, rows);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

int awq_launch_kv_dequant_fp8(const uint8_t* codes, const float* scales, uint16_t* out, int B, int n, int Hkv, int Tmax,
                              hipStream_t st) {
    if (B < 0 || n < 0 || Hkv < 1 || n > Tmax) return AWQ_ERR_BAD_SHAPE;
    const int64_t rows = (int64_t)B * n * Hkv;
    if (rows == 0) return AWQ_OK;
    hipLaunchKernelGGL(awq_kv_dequant_fp8_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, codes, scales,
                       reinterpret_cast<half_t*>(out), n, Hkv, Tmax, rows);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}
