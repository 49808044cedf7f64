// Shared by the paged GQA decode kernels (gqa_decode.hip, gqa_decode_wide.hip, gqa_sparse_decode.hip) and the indexers (gqa_block_score.hip,
// gqa_block_score_prefill.hip, lightning_indexer.hip; block_score_dev.h builds on it): the host helpers of the entry points, wave reductions,
// MFMA / packing helpers, the padded LDS row stride, the kernel parameter block and the kernel that merges flash-decoding partials.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "decode_plan.h"
#include "mi_sgl_kernels.h"

namespace mi_gqa {

// ---- host helpers of the C entry points
inline int padded_dim(int d) { return d <= 64 ? 64 : d <= 128 ? 128 : d <= 256 ? 256 : 0; }
inline int cus()                                                  // CUs of the current device (256 when it cannot be asked), asked once
{
    static int cached[64];
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 256;
    if (!cached[d]) {
        int n = 0;
        cached[d] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0) ? n : 256;
    }
    return cached[d];
}
// what every block-sparse entry point asks of its shapes: block size 16 / 32 / 64 / 128, head dim a multiple of 8 up to 256, bf16 / fp16,
// sm_scale > 0 (the scaling is applied before the maximum)
inline bool block_args_ok(int block_size, int head_dim, int dtype, float sm_scale)
{
    if (block_size != 16 && block_size != 32 && block_size != 64 && block_size != 128) return false;
    if (head_dim <= 0 || (head_dim % 8) || !padded_dim(head_dim)) return false;
    return (dtype == MI_DTYPE_BF16 || dtype == MI_DTYPE_F16) && sm_scale > 0.f;
}
inline bool aligned8(std::initializer_list<int64_t> strides)      // 16-byte loads of 2-byte elements
{
    for (const int64_t s : strides)
        if (s % 8) return false;
    return true;
}
// dtype, padded head dim and one more flag as compile-time constants: f(std::true_type{}, std::integral_constant<int, 128>{}, std::false_type{})
template <class F>
inline void dispatch(bool bf16, int dp, bool flag, F f)
{
    auto dims = [&](auto bf, auto fl) {
        if (dp == 64) f(bf, std::integral_constant<int, 64>{}, fl);
        else if (dp == 128) f(bf, std::integral_constant<int, 128>{}, fl);
        else f(bf, std::integral_constant<int, 256>{}, fl);
    };
    auto flags = [&](auto bf) { flag ? dims(bf, std::true_type{}) : dims(bf, std::false_type{}); };
    bf16 ? flags(std::true_type{}) : flags(std::false_type{});
}

// Reductions across the four 16-lane rows of a wave through v_permlane16_swap / v_permlane32_swap (VALU) instead of ds_bpermute (an LDS
// round trip each).  swap16(x): {rows 0,0,2,2 | rows 1,1,3,3} of x; swap32(x): {lower half twice | upper half twice}.  Sums and maxima of
// the two parts are the xor-16 / xor-32 butterfly steps (same two operands in every lane: bit-identical to the shuffle form).
struct RowPair {
    float a, b;
};
__device__ __forceinline__ RowPair swap16(float x)
{
    typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
    const unsigned u = __float_as_uint(x);
    const u32x2v r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return RowPair{__uint_as_float(r[0]), __uint_as_float(r[1])};
}
__device__ __forceinline__ RowPair swap32(float x)
{
    typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
    const unsigned u = __float_as_uint(x);
    const u32x2v r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return RowPair{__uint_as_float(r[0]), __uint_as_float(r[1])};
}
__device__ __forceinline__ float max_over_rows(float x)
{
    const RowPair p = swap16(x);
    const RowPair q = swap32(fmaxf(p.a, p.b));
    return fmaxf(q.a, q.b);
}
__device__ __forceinline__ float sum_over_rows(float x)
{
    const RowPair p = swap16(x);
    const RowPair q = swap32(p.a + p.b);
    return q.a + q.b;
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct GqaParams {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    const int32_t *seq_lens, *block_table;
    float *ws_o;      // [B][Hq][S][DVP] fp32 partial (unnormalised) outputs
    float *ws_ml;     // [B][Hq][S][2]   running max (scaled log2 domain), running sum
    int batch, q_heads, kv_heads, group, page_size, bt_stride, num_splits, lk, lv;
    int64_t q_sb, q_sh, k_sblk, k_srow, k_sh, v_sblk, v_srow, v_sh, o_sb, o_sh;
    float sm_scale;
    // attention with sinks (attention/sinks_attention.py:7-137, :139-286): a per-q-head logit that takes part in the softmax denominator only;
    // a sliding window (keys [len - window, len)); and, for the extend ("prefill") form, a row of the block table per query row
    const void *sinks;          // [q_heads], element type sinks_dtype (MI_DTYPE_*); null = none
    int sinks_dtype;
    int window;                 // -1 = all keys
    const int32_t *bt_rows;     // [batch] block-table row of every query row; null = row b
    // round 4: the length-aware work list of decode_plan.h (null = uniform num_splits): unit = item, its tile range and piece index come from
    // the list, its partial lives at slot (item, head of the group)
    const int32_t *plan;
    // two-piece sequences finished by their own workgroups (gqa_decode_wide.hip): the merge kernel re-arms the meeting words, returns at once
    // when need_merge does not carry this launch's tag, and skips heads whose finishing piece marked its sum (sign bit); null = plain merge
    uint64_t *pair_flags = nullptr, *need_merge = nullptr;
    uint64_t pair_tag = 0;
};
__device__ __forceinline__ float gqa_sink_l2(const GqaParams &p, int head)      // the sink logit in the kernel's log2 domain (NOT scaled by sm_scale)
{
    float v;
    if (p.sinks_dtype == MI_DTYPE_F32) v = ((const float *)p.sinks)[head];
    else if (p.sinks_dtype == MI_DTYPE_BF16) v = __uint_as_float((uint32_t)((const uint16_t *)p.sinks)[head] << 16);
    else v = (float)__builtin_bit_cast(_Float16, ((const uint16_t *)p.sinks)[head]);
    return v * 1.4426950408889634f;
}

template <bool BF16>
__device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c)
{
    if constexpr (BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <bool BF16>
__device__ __forceinline__ uint32_t pack2(float lo, float hi)
{
    if constexpr (BF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, f16x2));
}

constexpr int row_stride(int dim) { return dim * 2 + 32; }      // dim % 16 == 0 and (dim / 16) even -> odd count of 32-B units

// One staged tile of TILE keys (K rows of stride KS, then V rows of stride VS, in `buf`) against one block of 16 heads: S^T = K.Q^T on the
// MFMA, `mask(s)` writes -inf over the keys that take no part, online softmax in the scaled log2 domain (cs = sm_scale * log2 e), P rounded to
// the cache dtype, O^T += V^T.P^T.  Lane (g, c16) owns head c16 and keys mt*16 + 4g + r of the tile.
template <bool BF16, int DKP, int DVP, int TILE, class Mask>
__device__ __forceinline__ void tile_step(const uint8_t *buf, const s16x8 (&qf)[DKP / 32], f32x4 (&acc)[DVP / 16], float &m_run, float &l_run,
                                          float cs, int g, int c16, Mask mask)
{
    constexpr int KS = row_stride(DKP), VS = row_stride(DVP);
    constexpr int MT = TILE / 16, KK = TILE / 32, QS = DKP / 32, DT = DVP / 16;
    // ---- S^T[key, head] = K . Q^T
    f32x4 s[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) s[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < QS; ++ks)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const s16x8 a = *(const s16x8 *)(buf + (mt * 16 + c16) * KS + ks * 64 + g * 16);
            s[mt] = mfma16<BF16>(a, qf[ks], s[mt]);
        }
    // ---- online softmax in the scaled log2 domain; lane owns head c16 and keys mt*16 + 4g + r
    mask(s);
    float tmax = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) tmax = fmaxf(fmaxf(tmax, fmaxf(s[mt][0], s[mt][1])), fmaxf(s[mt][2], s[mt][3]));
    tmax = max_over_rows(tmax);
    tmax *= cs;                                           // sm_scale > 0: max commutes with the scaling
    if (__any(tmax > m_run)) {
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
        m_run = m_new;
#pragma unroll
        for (int i = 0; i < DT; ++i) acc[i] *= alpha;
    }
    const float nm = (m_run == -INFINITY) ? 0.f : -m_run;
    float psum = 0.f;
    uint32_t pk[MT * 2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[mt][r], cs, nm));
            psum += e[r];
        }
        pk[mt * 2 + 0] = pack2<BF16>(e[0], e[1]);
        pk[mt * 2 + 1] = pack2<BF16>(e[2], e[3]);
    }
    psum = sum_over_rows(psum);
    l_run += psum;
    // ---- O^T[d, head] += V^T . P^T ; k-step kk covers key tiles (2kk, 2kk+1): slots 0..3 / 4..7 of lane group g
    const uint8_t *vrow = buf + TILE * KS + (4 * g + (c16 >> 2)) * VS + (c16 & 3) * 8;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        const s16x8 pf = __builtin_bit_cast(s16x8, u32x4{pk[kk * 4 + 0], pk[kk * 4 + 1], pk[kk * 4 + 2], pk[kk * 4 + 3]});
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (s16x4 __attribute__((address_space(3))) *)(vrow + (2 * kk) * 16 * VS + dt * 32));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (s16x4 __attribute__((address_space(3))) *)(vrow + (2 * kk + 1) * 16 * VS + dt * 32));
            const s16x8 a = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            acc[dt] = mfma16<BF16>(a, pf, acc[dt]);
        }
    }
}

// merge the flash-decoding partials: one wave per (b, head); lane handles dims lane*4 + 256 i
// (static: both translation units launch it, each through its own copy, as with decode_plan.h's kernel)
template <bool BF16>
static __global__ __launch_bounds__(256) void gqa_merge_kernel(GqaParams p, int dvp)
{
    const int lane = threadIdx.x & 63;
    const int64_t bh = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (bh >= (int64_t)p.batch * p.q_heads) return;
    const int b = (int)(bh / p.q_heads), h = (int)(bh % p.q_heads);
    // the meeting words of the sequence's two pieces (gqa_decode_wide.hip) are re-armed here, behind the launch that used them: the next
    // call -- or the next replay of a captured one, which carries the same tag -- finds them clear
    if (p.pair_flags && h % p.group == 0 && lane < 2) p.pair_flags[((int64_t)b * p.kv_heads + h / p.group) * 2 + lane] = 0ull;
    // every sequence finished in the decode kernel (two pieces each, or one): one load per wave instead of the statistics round trips
    if (p.need_merge && __hip_atomic_load(p.need_merge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != p.pair_tag) return;
    // partial s of this head: slot (bh, s), or -- planned form -- slot (item of piece s, head within the group)
    int S = p.num_splits, first = 0;
    if (p.plan) {
        const int32_t *info = p.plan + mi_sgl::kPlanHdr + 2ll * (b * p.kv_heads + h / p.group);
        first = info[0], S = info[1];
        if (S == 1) return;                                   // the piece wrote the output row itself
    }
    auto slot = [&](int s) -> int64_t { return p.plan ? (int64_t)(first + s) * p.group + h % p.group : bh * S + s; };
    // two pieces: piece (head within the group) / 64 finished this head itself if its sum carries the mark (the sign); without the mark
    // (its partner did not show up in time) both partials of the head are complete in the workspace: merge as usual
    const bool marks = p.pair_flags != nullptr && S == 2;
    if (marks && (__float_as_uint(p.ws_ml[slot((h % p.group) >> 6) * 2 + 1]) >> 31)) return;
    auto sum_of = [&](int s) -> float { const float l = p.ws_ml[slot(s) * 2 + 1]; return marks ? fabsf(l) : l; };
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, p.ws_ml[slot(s) * 2]);
    const float sk = p.sinks ? gqa_sink_l2(p, h) : -INFINITY;
    M = fmaxf(M, sk);
    float L = p.sinks ? __builtin_amdgcn_exp2f(sk - M) : 0.f;
    // (explicit fused multiply-adds: gqa_decode_wide.hip's pair finish forms the same sums in the same order and must round the same way)
    for (int s = 0; s < S; ++s) {
        const float m = p.ws_ml[slot(s) * 2];
        if (m != -INFINITY) L = __builtin_fmaf(__builtin_amdgcn_exp2f(m - M), sum_of(s), L);
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
    uint16_t *orow = p.out + (int64_t)b * p.o_sb + (int64_t)h * p.o_sh;
    for (int d = lane * 4; d < p.lv; d += 256) {
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S; ++s) {
            const float m = p.ws_ml[slot(s) * 2];
            if (m == -INFINITY) continue;
            const float w = __builtin_amdgcn_exp2f(m - M);
            const f32x4 a = *(const f32x4 *)(p.ws_o + slot(s) * dvp + d);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = __builtin_fmaf(w, a[i], o[i]);
        }
        *(uint2 *)(orow + d) = uint2{pack2<BF16>(o[0] * inv, o[1] * inv), pack2<BF16>(o[2] * inv, o[3] * inv)};
    }
}

}  // namespace mi_gqa
