// Block-sparse grouped-query decode attention for gfx950: every sequence attends to the KV blocks its top-k list names.
// Replaces the reference's Triton-Ascend `_gqa_share_sparse_decode_bnsd_kernel` + `_merge_topk_attn_out_bnsd_kernel`
// (python/sgl_kernel_npu/sgl_kernel_npu/attention/gqa_share_sparse_attention.py:180-546, :635-878): q [B, Hq, D], K / V caches
// [pages, block_size, Hkv, D], topk_idx [Hkv, B, topk] logical block ids (-1 = none, anywhere in the list, duplicates count twice),
// pages through a block table or a request -> token-slot map, an optional vector sink [Hq, D] whose logit (q . sink) * sm_scale enters the
// softmax maximum and denominator once and has no value row.
//
// The inner loop is gqa_decode.hip's (gqa_common.h: S^T = K.Q^T and O^T += V^T.P^T on the MFMA, online softmax in the log2 domain, K / V
// tiles of 64 keys double buffered in LDS with the padded row stride); a workgroup of 4 waves owns one (sequence, kv head, chunk of the
// top-k list) and all query heads of the group, so every selected K / V byte leaves HBM once per kv head.  What differs is where a tile
// comes from: the chunk's slots are resolved ONCE, up front, into an LDS list (logical block, page) -- a slot that is -1 or starts at or
// behind the sequence's end is dropped there and its table entry is never read -- so the tile loop's loads depend on LDS only, not on an
// idx -> table -> row chain per tile.  The chunk's slots x block_size keys form one virtual key range cut in 64-key tiles: a block of 128
// keys is two tiles, four blocks of 16 keys share one; a key takes part when its LOGICAL position lies inside the sequence, wherever its
// block sits in the list; rows that take no part are staged as zeros and tiles without a single key are skipped.
// Chunks write fp32 partials (unnormalised o, running max, running sum) that gqa_decode.hip's merge kernel combines; the sink belongs to
// chunk 0.  The chunk count comes from the host, from shapes only: nothing is read back, the launches can be captured in a graph.
#include <algorithm>

#include "device_once.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_score_dev.h"
#include "mi_sgl_kernels.h"

namespace mi_gqa_sparse {
using namespace mi_gqa;

constexpr int kTile = 64;
constexpr int kMaxChunkSlots = 1024;      // list entries a workgroup keeps in LDS (8 B each) next to the two tile buffers

struct Params {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    const int32_t *seq_lens;
    const void *topk;               // [kv_heads, batch, topk] through the three strides
    int topk_i64;
    int64_t ti_sh, ti_sb, ti_st;
    PageMap pages;
    const void *sink;               // [q_heads, d], rows sink_sh apart; null = none
    int sink_dtype;
    int64_t sink_sh;
    float *ws_o, *ws_ml;            // [B][Hq][chunks][DP] unnormalised partial outputs; [B][Hq][chunks][2] running max (log2 domain), sum
    int batch, q_heads, kv_heads, group, block_size, bs_shift, topk_n, max_kv_len, num_chunks, chunk_slots, list_cap, d;
    int64_t q_sb, q_sh, k_sblk, k_srow, k_sh, v_sblk, v_srow, v_sh, o_sb, o_sh;
    float sm_scale;
};

__device__ __forceinline__ float load_elem(const void *base, int dtype, int64_t off)
{
    if (dtype == MI_DTYPE_F32) return ((const float *)base)[off];
    const uint16_t u = ((const uint16_t *)base)[off];
    return dtype == MI_DTYPE_BF16 ? __uint_as_float((uint32_t)u << 16) : (float)__builtin_bit_cast(_Float16, u);
}
template <bool BF16>
__device__ __forceinline__ float elem_f32(short x)
{
    if constexpr (BF16) return __uint_as_float((uint32_t)(uint16_t)x << 16);
    else return (float)__builtin_bit_cast(_Float16, x);
}

// DP: compile-time padded head dim (64, 128, 256); HB head blocks of 16 per wave (a workgroup covers 64 * HB heads of the group).
template <bool BF16, int DP, int HB>
__global__ __launch_bounds__(256) void gqa_sparse_decode_kernel(Params p)
{
    constexpr int TILE = kTile, KS = row_stride(DP), kBuf = TILE * 2 * KS;
    constexpr int MT = TILE / 16, QS = DP / 32, DT = DP / 16;
    constexpr int C = DP / 8, RP = TILE / 32, J = (C + 7) / 8;    // 16-B chunks per row; row passes (8 threads per row, 32 rows a pass)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    int32_t *s_lb = (int32_t *)(lds + 2 * kBuf), *s_pg = s_lb + p.list_cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    constexpr int kHeadsPerWg = 64 * HB;
    const int head_blocks = (p.group + kHeadsPerWg - 1) / kHeadsPerWg;
    int u = blockIdx.x;                                           // the grid is exactly batch * kv_heads * chunks * head_blocks
    const int hblk = u % head_blocks;
    u /= head_blocks;
    const int chunk = u % p.num_chunks;
    u /= p.num_chunks;
    const int kvh = u % p.kv_heads, b = u / p.kv_heads;
    const int BS = p.block_size, shift = p.bs_shift;
    const int seq_len = min(p.seq_lens[b], p.max_kv_len);

    // ---- the chunk's slots -> (logical block, page); -1 for a slot that names no block or one at / behind the sequence's end (its table
    // entry is not read: lb * BS < seq_len <= max_kv_len keeps every entry that IS read inside the table)
    const int s_begin = chunk * p.chunk_slots;
    const int n_slots = max(0, min(p.topk_n, s_begin + p.chunk_slots) - s_begin);
    for (int i = tid; i < p.list_cap; i += 256) {
        int32_t lb = -1, pg = 0;
        if (i < n_slots) {
            const int64_t l = load_index(p.topk, p.topk_i64, kvh * p.ti_sh + b * p.ti_sb + (int64_t)(s_begin + i) * p.ti_st);
            if (l >= 0 && l * BS < (int64_t)seq_len) lb = (int32_t)l, pg = (int32_t)page_of(p.pages, b, l, BS);
        }
        s_lb[i] = lb, s_pg[i] = pg;
    }

    // Q^T fragments: lane (g, c16) holds q[head][ks*32 + g*8 .. +8] of head block hb
    s16x8 qf[HB][QS];
    int hg[HB];
    bool wave_has[HB];
    f32x4 acc[HB][DT];
    float m_run[HB], l_run[HB];
    const float cs = p.sm_scale * 1.4426950408889634f;
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        hg[hb] = hblk * kHeadsPerWg + (hb * 4 + wave) * 16 + c16;
        wave_has[hb] = hblk * kHeadsPerWg + (hb * 4 + wave) * 16 < p.group;      // waves without a real head still help to stage tiles
        const bool ok = hg[hb] < p.group;
        const int head = kvh * p.group + (ok ? hg[hb] : 0);
        const uint16_t *qrow = p.q + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh;
#pragma unroll
        for (int ks = 0; ks < QS; ++ks) {
            const int d = ks * 32 + g * 8;
            qf[hb][ks] = (ok && d < p.d) ? *(const s16x8 *)(qrow + d) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        m_run[hb] = -INFINITY, l_run[hb] = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i) acc[hb][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the sink: one more logit, (q . sink) * sm_scale in fp32, counted once -- by chunk 0 -- as the state the online softmax starts from
        if (p.sink && chunk == 0 && wave_has[hb]) {               // wave-uniform
            float part = 0.f;
#pragma unroll
            for (int ks = 0; ks < QS; ++ks) {
                const int d = ks * 32 + g * 8;
                if (ok && d < p.d) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) part += elem_f32<BF16>(qf[hb][ks][i]) * load_elem(p.sink, p.sink_dtype, head * p.sink_sh + d + i);
                }
            }
            m_run[hb] = sum_over_rows(part) * cs;
            l_run[hb] = 1.f;
        }
    }
    __syncthreads();                                              // the list is complete

    // ---- tiles of the chunk's virtual key range [0, n_slots * BS): key j = slot j >> shift, row j & (BS - 1) of its block
    const int ntiles = (n_slots * BS + TILE - 1) / TILE;
    const int slots_per_tile = max(1, TILE >> shift);
    auto next_tile = [&](int t) {                                 // the first tile from t on with a key that takes part (the same in every thread)
        for (; t < ntiles; ++t) {
            const int first = (t * TILE) >> shift, n0 = (t * TILE) & (BS - 1);
            bool any = false;
            for (int i = 0; i < slots_per_tile; ++i) {
                const int lb = s_lb[first + i];                   // first + i < list_cap: the list is padded to whole tiles with -1
                any |= lb >= 0 && lb * BS + n0 < seq_len;
            }
            if (any) break;
        }
        return t;
    };

    u32x4 kreg[RP][J], vreg[RP][J];
    const int srow = tid >> 3, sch = tid & 7;
    auto stage_load = [&](int tile) {
#pragma unroll
        for (int rp = 0; rp < RP; ++rp) {
            const int j = tile * TILE + rp * 32 + srow, slot = j >> shift, n = j & (BS - 1);
            const int lb = s_lb[slot];
            const int64_t pg = s_pg[slot];
            const bool ok = lb >= 0 && lb * BS + n < seq_len;     // rows that take no part are zeros in LDS and are never read from the caches
            const uint16_t *kr = p.k + pg * p.k_sblk + (int64_t)n * p.k_srow + (int64_t)kvh * p.k_sh;
            const uint16_t *vr = p.v + pg * p.v_sblk + (int64_t)n * p.v_srow + (int64_t)kvh * p.v_sh;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                const int c = sch + 8 * jj;
                const bool in = ok && c * 8 < p.d;
                kreg[rp][jj] = in ? *(const u32x4 *)(kr + c * 8) : u32x4{0, 0, 0, 0};
                vreg[rp][jj] = in ? *(const u32x4 *)(vr + c * 8) : u32x4{0, 0, 0, 0};
            }
        }
    };
    auto stage_store = [&](uint8_t *buf) {
#pragma unroll
        for (int rp = 0; rp < RP; ++rp) {
            const int row = rp * 32 + srow;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                const int c = sch + 8 * jj;
                if (c < C) {
                    *(u32x4 *)(buf + row * KS + c * 16) = kreg[rp][jj];
                    *(u32x4 *)(buf + TILE * KS + row * KS + c * 16) = vreg[rp][jj];
                }
            }
        }
    };

    int t = next_tile(0), nbuf_i = 0;
    if (t < ntiles) {
        stage_load(t);
        stage_store(lds);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                           // nothing in flight when the tile loop starts (see gqa_decode.hip)
    while (t < ntiles) {
        uint8_t *buf = lds + nbuf_i * kBuf;
        uint8_t *nbuf = lds + (nbuf_i ^ 1) * kBuf;
        const int tn = next_tile(t + 1);
        const bool more = tn < ntiles;
        __syncthreads();                                          // tile t complete in LDS; the tile before it no longer read
        if (more) stage_load(tn);                                 // travels under this tile's MFMAs
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            if (!wave_has[hb]) continue;                          // wave-uniform
            tile_step<BF16, DP, DP, TILE>(buf, qf[hb], acc[hb], m_run[hb], l_run[hb], cs, g, c16, [&](f32x4(&s)[MT]) {
                // 16 keys of an MFMA row block lie in one block (BS >= 16): keys r < lim of this lane's four take part
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int j0 = t * TILE + mt * 16;
                    const int lb = s_lb[j0 >> shift];
                    const int lim = lb < 0 ? 0 : seq_len - lb * BS - ((j0 & (BS - 1)) + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r >= lim) s[mt][r] = -INFINITY;
                }
            });
        }
        if (more) stage_store(nbuf);
        t = tn, nbuf_i ^= 1;
    }

    // ---- epilogue: lane holds O^T[d = dt*16 + 4g + r][head c16]
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        if (hg[hb] >= p.group) continue;
        const int head = kvh * p.group + hg[hb];
        if (p.num_chunks == 1) {
            const float inv = l_run[hb] > 0.f ? 1.f / l_run[hb] : 0.f;      // no key at all: zeros (with a sink too: acc = 0)
            uint16_t *orow = p.out + (int64_t)b * p.o_sb + (int64_t)head * p.o_sh + 4 * g;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (dt * 16 + 4 * g >= p.d) continue;             // d % 8 == 0: the 4 dims are in or out together
                const uint32_t w0 = pack2<BF16>(acc[hb][dt][0] * inv, acc[hb][dt][1] * inv);
                const uint32_t w1 = pack2<BF16>(acc[hb][dt][2] * inv, acc[hb][dt][3] * inv);
                *(uint2 *)(orow + dt * 16) = uint2{w0, w1};
            }
        } else {
            const int64_t idx = ((int64_t)b * p.q_heads + head) * p.num_chunks + chunk;
            float *po = p.ws_o + idx * DP + 4 * g;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) *(f32x4 *)(po + dt * 16) = acc[hb][dt];
            if (g == 0) {
                p.ws_ml[idx * 2 + 0] = m_run[hb];
                p.ws_ml[idx * 2 + 1] = l_run[hb];
            }
        }
    }
}

template <bool BF16, int DP, int HB>
static void launch_one(const Params &p, unsigned grid, hipStream_t st)
{
    constexpr size_t tiles = 2 * (size_t)kTile * 2 * row_stride(DP);
    static PerDeviceOnce attr_once;
    if (attr_once.need()) {
        (void)hipFuncSetAttribute((const void *)gqa_sparse_decode_kernel<BF16, DP, HB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(tiles + 2 * sizeof(int32_t) * kMaxChunkSlots));
    }
    gqa_sparse_decode_kernel<BF16, DP, HB><<<grid, 256, tiles + 2 * sizeof(int32_t) * p.list_cap, st>>>(p);
}

}  // namespace mi_gqa_sparse

using namespace mi_gqa_sparse;

extern "C" size_t mi_gqa_sparse_decode_workspace(int batch, int q_heads, int head_dim, int num_chunks)
{
    const int dp = padded_dim(head_dim);
    if (batch <= 0 || q_heads <= 0 || head_dim <= 0 || !dp || num_chunks <= 1) return 0;
    return (size_t)batch * q_heads * num_chunks * (dp + 2) * sizeof(float);
}

// Chunks of the top-k list per (sequence, kv head): a power of two that brings the grid to about two workgroups per CU, at most the list's
// length and 64.  From shapes and the CU count only.
extern "C" int mi_gqa_sparse_decode_num_chunks(int batch, int kv_heads, int topk)
{
    if (batch <= 0 || kv_heads <= 0 || topk <= 1) return 1;
    const long long wgs = (long long)batch * kv_heads;
    const long long want = std::min<long long>(std::min<long long>((2ll * cus() + wgs - 1) / wgs, topk), 64);
    int c = 1;
    while (2 * c <= want) c *= 2;
    return c;
}

extern "C" int mi_gqa_sparse_decode(const void *q, const void *k, const void *v, void *out, const int32_t *seq_lens, const void *topk_idx,
                                    int topk_is_i64, int64_t topk_stride_h, int64_t topk_stride_b, int64_t topk_stride_t,
                                    const void *block_table, int block_table_is_i64, int64_t bt_stride_b, int64_t bt_stride_n,
                                    const void *req_to_token, int req_to_token_is_i64, int64_t rtt_stride_r, int64_t rtt_stride_t,
                                    int rtt_cols, const void *req_pool_indices, int req_pool_is_i64, const void *sink, int sink_dtype,
                                    int64_t sink_stride_h, int batch, int q_heads, int kv_heads, int head_dim, int block_size, int topk,
                                    int max_kv_len, int num_pages, int sanitize_page_ids, int64_t q_stride_b, int64_t q_stride_h,
                                    int64_t k_stride_blk, int64_t k_stride_row, int64_t k_stride_h, int64_t v_stride_blk,
                                    int64_t v_stride_row, int64_t v_stride_h, int64_t o_stride_b, int64_t o_stride_h, float sm_scale,
                                    int dtype, int num_chunks, void *workspace, size_t workspace_bytes, void *stream)
{
    if (batch < 0 || q_heads <= 0 || kv_heads <= 0 || q_heads % kv_heads || topk < 0 || max_kv_len < 0) return MI_SGL_EINVAL;
    if (!block_args_ok(block_size, head_dim, dtype, sm_scale)) return MI_SGL_EINVAL;
    const int dp = padded_dim(head_dim);
    if (sink && sink_dtype != MI_DTYPE_BF16 && sink_dtype != MI_DTYPE_F16 && sink_dtype != MI_DTYPE_F32) return MI_SGL_EINVAL;
    // exactly one page source
    const bool direct = req_to_token != nullptr;
    if (direct == (block_table != nullptr) || direct != (req_pool_indices != nullptr)) return MI_SGL_EINVAL;
    if (direct && (rtt_cols <= 0 || num_pages <= 0)) return MI_SGL_EINVAL;
    if (num_chunks == 0) num_chunks = mi_gqa_sparse_decode_num_chunks(batch, kv_heads, topk);
    if (num_chunks < 0 || num_chunks > std::max(1, topk)) return MI_SGL_EINVAL;
    const int chunk_slots = (topk + num_chunks - 1) / num_chunks;
    if (chunk_slots > kMaxChunkSlots) return MI_SGL_ENOTAPPLICABLE;   // more chunks bring a longer list into reach
    if (batch == 0) return MI_SGL_OK;
    if (!q || !k || !v || !out || !seq_lens || (topk > 0 && !topk_idx)) return MI_SGL_EINVAL;
    if (!aligned8({q_stride_h, q_stride_b, k_stride_row, k_stride_blk, k_stride_h, v_stride_row, v_stride_blk, v_stride_h}) ||
        (o_stride_h % 4) || (o_stride_b % 4))
        return MI_SGL_EINVAL;      // 16-byte loads, 8-byte stores
    if (num_chunks > 1 && (!workspace || ((uintptr_t)workspace & 15) ||
                           workspace_bytes < mi_gqa_sparse_decode_workspace(batch, q_heads, head_dim, num_chunks)))
        return MI_SGL_EINVAL;
    Params p;
    p.q = (const uint16_t *)q, p.k = (const uint16_t *)k, p.v = (const uint16_t *)v, p.out = (uint16_t *)out, p.seq_lens = seq_lens;
    p.topk = topk_idx, p.topk_i64 = topk_is_i64, p.ti_sh = topk_stride_h, p.ti_sb = topk_stride_b, p.ti_st = topk_stride_t;
    p.pages = make_page_map(block_table, block_table_is_i64, bt_stride_b, bt_stride_n, req_to_token, req_to_token_is_i64, rtt_stride_r,
                            rtt_stride_t, rtt_cols, req_pool_indices, req_pool_is_i64, num_pages, sanitize_page_ids);
    p.sink = sink, p.sink_dtype = sink_dtype, p.sink_sh = sink_stride_h;
    p.ws_o = (float *)workspace;
    p.ws_ml = p.ws_o ? p.ws_o + (size_t)batch * q_heads * num_chunks * dp : nullptr;
    p.batch = batch, p.q_heads = q_heads, p.kv_heads = kv_heads, p.group = q_heads / kv_heads, p.block_size = block_size;
    p.bs_shift = __builtin_ctz(block_size), p.topk_n = topk, p.max_kv_len = max_kv_len, p.num_chunks = num_chunks;
    p.chunk_slots = chunk_slots, p.list_cap = (chunk_slots + 3) / 4 * 4, p.d = head_dim;
    p.q_sb = q_stride_b, p.q_sh = q_stride_h, p.k_sblk = k_stride_blk, p.k_srow = k_stride_row, p.k_sh = k_stride_h;
    p.v_sblk = v_stride_blk, p.v_srow = v_stride_row, p.v_sh = v_stride_h, p.o_sb = o_stride_b, p.o_sh = o_stride_h;
    p.sm_scale = sm_scale;
    const int hpw = p.group <= 64 ? 64 : 128;
    const int head_blocks = (p.group + hpw - 1) / hpw;
    const long long wgs = (long long)batch * kv_heads * num_chunks * head_blocks;
    if (wgs > 0x7fffffffll) return MI_SGL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool bf16 = dtype == MI_DTYPE_BF16;
    dispatch(bf16, dp, hpw == 64, [&](auto bf, auto d, auto one) { launch_one<bf(), d(), one() ? 1 : 2>(p, (unsigned)wgs, st); });
    if (num_chunks > 1) {
        GqaParams m{};                                            // the merge kernel of gqa_decode.hip on this kernel's partial layout
        m.out = (uint16_t *)out, m.ws_o = p.ws_o, m.ws_ml = p.ws_ml, m.batch = batch, m.q_heads = q_heads, m.kv_heads = kv_heads;
        m.group = p.group, m.num_splits = num_chunks, m.lv = head_dim, m.o_sb = o_stride_b, m.o_sh = o_stride_h;
        m.plan = nullptr, m.sinks = nullptr, m.window = -1, m.bt_rows = nullptr;
        const int blocks = (int)(((long long)batch * q_heads + 3) / 4);
        if (bf16) gqa_merge_kernel<true><<<blocks, 256, 0, st>>>(m, dp);
        else gqa_merge_kernel<false><<<blocks, 256, 0, st>>>(m, dp);
    }
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}
