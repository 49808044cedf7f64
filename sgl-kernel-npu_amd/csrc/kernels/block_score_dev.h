// Shared by the block-sparse family (gqa_block_score.hip, gqa_block_score_prefill.hip, gqa_sparse_decode.hip; lightning_indexer.hip takes the
// sort): the logical block -> page lookup, the 46-bit selection key, the block-score engine both score kernels are a front end of, and the
// LDS bitonic sort of 64-bit keys.
#pragma once
#include "gqa_common.h"

namespace mi_gqa {

constexpr int kMaxSeqBlock = 16384, kIdxBits = 14, kMaxTopk = 1024;
static_assert((1 << kIdxBits) == kMaxSeqBlock, "a block id fills the key's low bits");
inline bool within_limits(int max_seqblock, int topk) { return max_seqblock > 0 && max_seqblock <= kMaxSeqBlock && topk > 0 && topk <= kMaxTopk; }

__device__ __forceinline__ int64_t load_index(const void *base, int is_i64, int64_t off)
{
    return is_i64 ? ((const int64_t *)base)[off] : (int64_t)((const int32_t *)base)[off];
}

__device__ __forceinline__ uint64_t block_key(float score, int j)      // smaller = better: higher score first, then the lower block id
{
    const uint32_t u = __float_as_uint(score);
    const uint32_t asc = (u >> 31) ? ~u : (u | 0x80000000u);
    return ((uint64_t)(~asc) << kIdxBits) | (uint32_t)j;
}

// ---- where the page of a logical block comes from
struct PageMap {
    const void *table;              // block_table [batch, columns], or req_to_token [requests, cols] when req_pool is set
    int table_i64;
    int64_t tb_sr, tb_sc;
    const void *req_pool;           // [batch]; null = block-table form
    int req_i64, rtt_cols, num_pages, sanitize;     // num_pages / sanitize: the clamp of page_of's req_to_token form only, never page_of_row's
};
inline PageMap make_page_map(const void *block_table, int bt_i64, int64_t bt_sr, int64_t bt_sc, const void *req_to_token, int rtt_i64,
                             int64_t rtt_sr, int64_t rtt_sc, int rtt_cols, const void *req_pool, int req_i64, int num_pages, int sanitize)
{
    if (req_to_token) return PageMap{req_to_token, rtt_i64, rtt_sr, rtt_sc, req_pool, req_i64, rtt_cols, num_pages, sanitize};
    return PageMap{block_table, bt_i64, bt_sr, bt_sc, nullptr, 0, rtt_cols, num_pages, sanitize};
}
// req_to_token form, the request's pool row already loaded: the token slot of the block's first key (column clamped into the row) / BS
__device__ __forceinline__ int64_t page_of_row(const PageMap &m, int64_t pool_row, int64_t blk, int BS)
{
    const int64_t col = min(blk * BS, (int64_t)m.rtt_cols - 1);
    return load_index(m.table, m.table_i64, pool_row * m.tb_sr + col * m.tb_sc) / BS;
}
// either form for sequence b; the caller keeps blk inside the table
__device__ __forceinline__ int64_t page_of(const PageMap &m, int b, int64_t blk, int BS)
{
    if (!m.req_pool) return load_index(m.table, m.table_i64, b * m.tb_sr + blk * m.tb_sc);
    const int64_t page = page_of_row(m, load_index(m.req_pool, m.req_i64, b), blk, BS);
    return m.sanitize ? min(max(page, (int64_t)0), (int64_t)m.num_pages - 1) : page;
}

// ---- the score engine: what a wave does with its logical blocks jw, jw + 4, ... < j1 (jw < j1) of one kv head against NB blocks of 16
// columns (query heads, or (token, head) pairs) whose Q^T fragments qf it holds: lane (g, c16) holds dims ks*32 + 8g .. +8 of column c16.
// No V, no accumulator, no LDS, no barrier.  Column nb sees the keys at positions below lim[nb]; rows at or behind load_lim (>= every lim)
// are zeros that are never read; blocks that end at or below lim_min (<= every lim; 0 = none) skip the per-row mask.  page_of(j) is the
// page of block j, store(nb, j, score) receives -- in the lanes g == 0, column c16 -- the block's maximum or (LSE) log-sum-exp, fp32 in the
// log2 domain of cs = sm_scale * log2 e.
struct KeyRows {
    const uint16_t *k;              // the kv head's row 0 of page 0
    int64_t sblk, srow;
    int d, block_size, bs_shift;
};
template <bool BF16, int DP, int NB, bool LSE, class PageOf, class Store>
__device__ __forceinline__ void score_blocks(const KeyRows &kc, int jw, int j1, const s16x8 (&qf)[NB][DP / 32], const int (&lim)[NB], int load_lim,
                                             int lim_min, float cs, PageOf page_of, Store store)
{
    constexpr int QS = DP / 32, UP = DP <= 128 ? 4 : 2;           // k-steps of a key row; 16-key units of a load stage
    const int lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    const int BS = kc.block_size, ushift = kc.bs_shift - 4, units = BS >> 4;
    const int T = __builtin_amdgcn_readfirstlane(((j1 - jw + 3) >> 2) << ushift);      // 16-key units of this wave

    // unit t of the wave: rows 16 (t mod units) .. +16 of block jw + 4 (t / units); lane loads dims ks*32 + 8g .. +8 of row c16.  The pages of
    // a stage's units are looked up by its first lanes (one vector load for the stage, not a scalar chain per unit) and read lane by lane.
    auto load_stage = [&](int t0, u32x4(&kr)[UP][QS]) {
        const int tl = t0 + (lane & (UP - 1)), jl = jw + 4 * (tl >> ushift);
        const int page_l = tl < T ? (int)page_of(jl) : 0;         // jl < j1: inside the table
#pragma unroll
        for (int i = 0; i < UP; ++i) {
            const int t = t0 + i;
            const int j = jw + 4 * (t >> ushift), n = ((t & (units - 1)) << 4) + c16;
            const int64_t page = __builtin_amdgcn_readlane(page_l, i);
            const bool ok = t < T && j * BS + n < load_lim;
            const uint16_t *krow = kc.k + page * kc.sblk + (int64_t)n * kc.srow;
#pragma unroll
            for (int ks = 0; ks < QS; ++ks) {
                const int d = ks * 32 + g * 8;
                kr[i][ks] = (ok && d < kc.d) ? *(const u32x4 *)(krow + d) : u32x4{0, 0, 0, 0};
            }
        }
    };

    // per lane and column block: running maximum and (LSE) exp2 sum over the lane's keys 4g + r of the block's units seen so far
    float m_run[NB], l_run[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) m_run[nb] = -INFINITY, l_run[nb] = 0.f;

    auto compute_stage = [&](int t0, const u32x4(&kr)[UP][QS]) {
#pragma unroll
        for (int i = 0; i < UP; ++i) {
            const int t = t0 + i;
            if (t >= T) break;                                    // wave-uniform
            const int j = jw + 4 * (t >> ushift), un = t & (units - 1);
            const int pos0 = j * BS + (un << 4) + 4 * g;          // logical position of this lane's key r = 0
            const bool front = lim_min > 0 && (j + 1) * BS <= lim_min;      // wave-uniform: every column sees the whole block
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < QS; ++ks) s = mfma16<BF16>(__builtin_bit_cast(s16x8, kr[i][ks]), qf[nb][ks], s);
                float v[4];
                if (front) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = s[r] * cs;
                } else {
                    const int left = lim[nb] - pos0;              // keys r < left take part
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = r < left ? s[r] * cs : -INFINITY;
                }
                const float um = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                const float m_new = fmaxf(m_run[nb], um);
                if constexpr (LSE) {
                    if (m_new > -INFINITY) {
                        float e = l_run[nb] * __builtin_amdgcn_exp2f(m_run[nb] - m_new);
#pragma unroll
                        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(v[r] - m_new);
                        l_run[nb] = e;
                    }
                }
                m_run[nb] = m_new;
            }
            if (un == units - 1) {                                // the block is complete: the four lane rows meet
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const float M = max_over_rows(m_run[nb]);
                    float score = M;
                    if constexpr (LSE) {
                        const float part = M > -INFINITY ? l_run[nb] * __builtin_amdgcn_exp2f(m_run[nb] - M) : 0.f;
                        score = M + __builtin_amdgcn_logf(sum_over_rows(part));
                        if (score != score) score = -INFINITY;
                    }
                    if (g == 0) store(nb, j, score);
                    m_run[nb] = -INFINITY, l_run[nb] = 0.f;
                }
            }
        }
    };

    u32x4 ka[UP][QS], kb[UP][QS];
    load_stage(0, ka);
    for (int t0 = 0; t0 < T; t0 += 2 * UP) {
        load_stage(t0 + UP, kb);                                  // travels under the MFMAs of the stage before it
        compute_stage(t0, ka);
        load_stage(t0 + 2 * UP, ka);
        compute_stage(t0 + UP, kb);
    }
}

// ---- cand[0 .. P) ascending in LDS, P a power of two, by a workgroup of THREADS; cand is complete (a barrier passed) on entry and on return
template <int THREADS>
__device__ __forceinline__ void bitonic_sort(uint64_t *cand, int P)
{
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (P >> 1); i += THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const uint64_t a = cand[lo], c = cand[hi];
                if ((a > c) == ((lo & size) == 0)) cand[lo] = c, cand[hi] = a;
            }
            __syncthreads();
        }
}

}  // namespace mi_gqa
