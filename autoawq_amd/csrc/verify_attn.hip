// verify_attn.hip -- attention of T = 2 .. 8 NEW tokens per sequence over the cache, at per-row device positions
// (awq_verify_attention_rows, include/awq_hip.h): the middle of a speculative decode step.  awq_rope_kv_append_rows(S = T) has
// already written cache rows pos_b .. pos_b + T - 1; query (b, j) sees rows t <= pos_b + j.
//
// The kernel is awq_decode_attn_kernel's ROWS form (decoder.hip) with one more axis.  To that kernel a query token is what a second
// query head on the same KV head is: a cache row is loaded once -- 16 lanes x 16 bytes -- and scored against every (head, token)
// PAIR the block owns; the only new thing per pair is its visibility limit t <= pos_b + j.  Same geometry otherwise: 256 threads,
// lane (r, c) reads bytes [16c, 16c + 16) of row t0 + 4 (wave + 4 i) + r, 16-lane butterfly, online softmax per lane group,
// (max, sum, acc) merges over lane groups, waves and splits, rows dealt to the splits on the device from pos_b + T.
//
// Tiling of the G * T pairs: a block holds P = G * TT <= 8 pairs in registers -- exactly the qf[8][8] / o[8][8]
// footprint of the decode kernel's G = 8 instantiation, so the occupancy of the kernel it is derived from is kept -- and the
// ceil(T / TT) token groups ride on blockIdx.z beside the sequence.  Groups of one (KV head, sequence) re-read the rows from L2
// (the rows of one KV head at 2048 tokens are 1 MiB; a group's blocks are adjacent in the grid).  TT is the smallest power of two
// >= T that fits; pair slots past T are dead: they see no row and write nothing.
#include "awq_device.h"
#include "awq_internal.h"

namespace {

template <int CTRL>
AWQ_DEV float vdpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// sum over the 16 lanes of a row, in every lane (decoder.hip: row16_sum; DPP in single-split launches, butterflies otherwise)
AWQ_DEV float vrow16_sum(float s, bool dpp) {
    if (!dpp) {
#pragma unroll
        for (int x = 8; x > 0; x >>= 1) s += __shfl_xor(s, x, 64);
        return s;
    }
    s += vdpp_f<0xB1>(s);
    s += vdpp_f<0x4E>(s);
    s += vdpp_f<0x124>(s);
    s += vdpp_f<0x128>(s);
    return s;
}

// grid (splits, Hkv, B * NG), NG = ceil(T / TT) token groups; 256 threads.  Pair p = g * TT + jj: query head hk * G + g, token
// j = tg * TT + jj.  q / out [B, T, Hq, 128]; part [B * T * Hq, splits, 130] fp32.
template <int G, int TT>
__global__ __launch_bounds__(256) void awq_verify_attn_kernel(const half_t* __restrict__ q, const half_t* __restrict__ kc,
                                                             const half_t* __restrict__ vc, half_t* __restrict__ out,
                                                             float* __restrict__ part, const int* __restrict__ pos_rows, int T,
                                                             int NG, int Hq, int Hkv, int Tmax, float scale) {
    constexpr int D = 128, P = G * TT, U = 4;
    static_assert(P <= 8, "at most 8 (head, token) pairs per block");
    __shared__ float sm[4][P][D + 2];
    const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z / NG, tg = blockIdx.z % NG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane >> 4, c = lane & 15;
    const int64_t rowstride = (int64_t)Hkv * D;
    const half_t* kb = kc + ((int64_t)b * Tmax * Hkv + hk) * D + 8 * c;
    const half_t* vb = vc + ((int64_t)b * Tmax * Hkv + hk) * D + 8 * c;
    // one split: the first row sets are requested before the position has made its round trip (decoder.hip, `early`); rows past the
    // visible ones are requested too -- they exist, the cache is Tmax rows -- and never used
    const bool early = gridDim.x == 1;
    half8_t kv0[U], vv0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = 4 * wave + 16 * u + r;
        kv0[u] = half8_t{};
        vv0[u] = kv0[u];
        if (early && t < Tmax) {
            kv0[u] = *reinterpret_cast<const half8_t*>(kb + (int64_t)t * rowstride);
            vv0[u] = *reinterpret_cast<const half8_t*>(vb + (int64_t)t * rowstride);
        }
    }
    // device-side positions are clamped to the cache exactly as awq_rope_kv_append_rows clamps the rows it writes
    const int pos_b = pos_rows[b];
    int lim[TT];  // newest row token jj of this group may see; -1: a dead slot (j >= T)
#pragma unroll
    for (int jj = 0; jj < TT; ++jj) {
        const int j = tg * TT + jj;
        lim[jj] = j < T ? max(0, min(pos_b + j, Tmax - 1)) : -1;
    }
    const int len = max(0, min(pos_b + T - 1, Tmax - 1)) + 1;  // rows the SEQUENCE attends over: what the splits are dealt from
    const int chunk = (((len + (int)gridDim.x - 1) / (int)gridDim.x) + 15) & ~15;
    const int jlast = min(T, tg * TT + TT) - 1;                                    // the group's newest live token
    const int t0 = split * chunk, t1 = min(min(len, t0 + chunk), max(0, min(pos_b + jlast, Tmax - 1)) + 1);

    float qf[P][8];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int g = p / TT, j = min(tg * TT + p % TT, T - 1);  // (a dead slot reads the last token's query and never uses it)
        const half8_t qv = *reinterpret_cast<const half8_t*>(q + (((int64_t)b * T + j) * Hq + hk * G + g) * D + 8 * c);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[p][e] = (float)qv[e] * scale;
    }
    float m[P], l[P], o[P][8];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        m[p] = -INFINITY;
        l[p] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[p][e] = 0.f;
    }
    for (int tb = t0 + 4 * wave; tb < t1; tb += 16 * U) {  // wave-uniform trip count
        half8_t kv[U], vv[U];
        const bool first = early && tb == 4 * wave;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = tb + 16 * u + r;
            kv[u] = kv0[u];
            vv[u] = vv0[u];
            if (!first) {
                kv[u] = half8_t{};
                vv[u] = kv[u];
                if (t < t1) {
                    kv[u] = *reinterpret_cast<const half8_t*>(kb + (int64_t)t * rowstride);
                    vv[u] = *reinterpret_cast<const half8_t*>(vb + (int64_t)t * rowstride);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = tb + 16 * u + r;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) s += qf[p][e] * (float)kv[u][e];
                s = vrow16_sum(s, early);
                if (t < t1 && t <= lim[p % TT]) {  // the causal edge inside the T new rows
                    const float mn = fmaxf(m[p], s);
                    const float corr = __expf(m[p] - mn), pw = __expf(s - mn);
                    l[p] = l[p] * corr + pw;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[p][e] = o[p][e] * corr + pw * (float)vv[u][e];
                    m[p] = mn;
                }
            }
        }
    }
    // merge the four lane groups of the wave (lanes c, c + 16, c + 32, c + 48 hold the same dims)
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
            const float mo = __shfl_xor(m[p], x, 64), lo = __shfl_xor(l[p], x, 64);
            const float mn = fmaxf(m[p], mo);
            const float ca = (m[p] == -INFINITY) ? 0.f : __expf(m[p] - mn), cb = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[p][e] = o[p][e] * ca + __shfl_xor(o[p][e], x, 64) * cb;
            l[p] = l[p] * ca + lo * cb;
            m[p] = mn;
        }
        if (r == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[wave][p][8 * c + e] = o[p][e];
            if (c == 0) {
                sm[wave][p][D] = m[p];
                sm[wave][p][D + 1] = l[p];
            }
        }
    }
    __syncthreads();
    // merge the four waves: thread (p, d); a split that got no visible row of a pair writes the (-inf, 0) partial
    const int nsplit = gridDim.x;
    for (int idx = tid; idx < P * D; idx += 256) {
        const int p = idx / D, d = idx % D;
        const int g = p / TT, j = tg * TT + p % TT;
        if (j >= T) continue;
        float mn = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mn = fmaxf(mn, sm[w][p][D]);
        float acc = 0.f, ls = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float cw = (sm[w][p][D] == -INFINITY) ? 0.f : __expf(sm[w][p][D] - mn);
            acc += sm[w][p][d] * cw;
            ls += sm[w][p][D + 1] * cw;
        }
        const int64_t head = ((int64_t)b * T + j) * Hq + hk * G + g;
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

// The twin of awq_decode_attn_combine_kernel (decoder.hip), one block per (sequence, token, query head): lanes of wave 0 take
// one split each, then thread d adds the splits' accumulators.
__global__ __launch_bounds__(128) void awq_verify_attn_combine_kernel(const float* __restrict__ part, half_t* __restrict__ out,
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
        float tot = ls * w;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
        if (d == 0) denom = tot;
    }
    __syncthreads();
    float acc = 0.f;
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) acc += pp[s * (D + 2) + d] * wgt[s];
    out[head * D + d] = (half_t)(denom > 0.f ? acc / denom : 0.f);
}

template <int G, int TT>
void launch_verify(const AwqAttnArgs& a, dim3 grid, int T, int NG) {
    hipLaunchKernelGGL((awq_verify_attn_kernel<G, TT>), grid, dim3(256), 0, a.stream, reinterpret_cast<const half_t*>(a.q),
                       static_cast<const half_t*>(a.k_cache), static_cast<const half_t*>(a.v_cache), reinterpret_cast<half_t*>(a.out),
                       static_cast<float*>(a.workspace), a.len_dev, T, NG, (int)a.Hq, (int)a.Hkv, (int)a.Tmax, a.scale);
}

}  // namespace

// tokens of one block: the smallest power of two >= T with G * TT <= 8
static int verify_group_tokens(int G, int T) {
    int tt = 1;
    while (tt < T && G * tt * 2 <= 8) tt *= 2;
    return tt;
}

// token groups of one sequence: each is a block per split and KV head
static int verify_groups(int G, int T) { return (T + verify_group_tokens(G, T) - 1) / verify_group_tokens(G, T); }

int awq_verify_attention_splits_impl(int max_len, int B, int T, int Hq, int Hkv) {
    return awq_attn_splits(max_len, (int64_t)B * Hkv * verify_groups(Hq / Hkv, T));
}

size_t awq_verify_attention_workspace_bytes_impl(int B, int T, int Hq, int splits) {
    return (size_t)B * T * Hq * splits * (128 + 2) * sizeof(float);
}

int awq_launch_verify_attention(const AwqAttnArgs& a, int T) {
    const int max_len = (int)a.max_len, B = (int)a.B, Hq = (int)a.Hq, Hkv = (int)a.Hkv, Tmax = (int)a.Tmax;
    if (!a.len_dev) return AWQ_ERR_NULL;
    if (B < 0 || Hq < 1 || Hkv < 1 || Hq % Hkv || Tmax < 1) return AWQ_ERR_BAD_SHAPE;
    if ((int)a.D != 128 || T < 2 || T > 8) return AWQ_ERR_UNSUPPORTED;
    const int G = Hq / Hkv;
    if (!(G == 1 || G == 2 || G == 4 || G == 8)) return AWQ_ERR_UNSUPPORTED;
    if (max_len < T || max_len > Tmax) return AWQ_ERR_BAD_SHAPE;
    if (B == 0) return AWQ_OK;
    const int TT = verify_group_tokens(G, T), NG = verify_groups(G, T);
    if ((int64_t)B * NG > 65535) return AWQ_ERR_BAD_SHAPE;
    const int splits = awq_attn_splits(max_len, (int64_t)B * Hkv * NG, a.workspace ? a.workspace_bytes : 0,
                                       awq_verify_attention_workspace_bytes_impl(B, T, Hq, 1));
    const dim3 grid((unsigned)splits, (unsigned)Hkv, (unsigned)(B * NG));
#define AWQ_VERIFY_CASE(GG, TTT) \
    if (G == GG && TT == TTT) launch_verify<GG, TTT>(a, grid, T, NG);
    AWQ_VERIFY_CASE(1, 2)
    AWQ_VERIFY_CASE(1, 4)
    AWQ_VERIFY_CASE(1, 8)
    AWQ_VERIFY_CASE(2, 2)
    AWQ_VERIFY_CASE(2, 4)
    AWQ_VERIFY_CASE(4, 2)
    AWQ_VERIFY_CASE(8, 1)
#undef AWQ_VERIFY_CASE
    if (hipGetLastError() != hipSuccess) return AWQ_ERR_LAUNCH;
    if (splits > 1) {
        hipLaunchKernelGGL(awq_verify_attn_combine_kernel, dim3((unsigned)((int64_t)B * T * Hq)), dim3(128), 0, a.stream,
                           static_cast<float*>(a.workspace), reinterpret_cast<half_t*>(a.out), splits);
        if (hipGetLastError() != hipSuccess) return AWQ_ERR_LAUNCH;
    }
    return AWQ_OK;
}
