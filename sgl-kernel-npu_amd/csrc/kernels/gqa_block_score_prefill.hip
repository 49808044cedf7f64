// Block-score indexer of the block-sparse PREFILL for gfx950: which KV blocks should every query token of a chunk attend to?  Replaces the
// reference's Triton-Ascend python/sgl_kernel_npu/sgl_kernel_npu/indexer/flash_block_score_prefill.py (:21-220 score kernel, :383-431 the
// per-q-block mappings it precomputes, :673-811 top-k from the score with the causal-local append, :865-909 the entry point).  Produces the
// topk_idx [1, total_q, topk + 1] that the block-sparse prefill attention (fia_blockq_sparse_prefill) consumes.
//
// Two launches, both sized from host integers (total_q, the request count, max_seqblock, shapes) only -- nothing is read back, the ops replay
// in a graph:
//
//  score   a workgroup of 4 waves owns (a tile of TQ consecutive tokens of ONE request, a kv head, a run of logical KV blocks).  TQ x group
//          rows (token-major, TQ = 64 / group) are flattened into four 16-row MFMA column blocks whose Q^T fragments every wave keeps in
//          registers; wave w takes the run's blocks w, w + 4, ...  A 16-key unit of K is loaded straight into the A operand of
//          mfma_f32_16x16x32 (score_blocks of block_score_dev.h, the engine gqa_block_score_kernel runs too: no V, no P.V, no accumulator,
//          no LDS, no barrier) and multiplied into all four column blocks; the per-lane online maximum / exp2 sum is fp32 in the log2 domain
//          and the four lane rows meet in permlane swaps when a block ends.  The grid is the host bound ceil(total_q / TQ) + requests tiles
//          (the tokens behind the last request count as one more request); a workgroup finds its request and tile by walking cu_seqlens.
//          Pages come straight from req_to_token: neither the reference's per-q-block mapping tensors nor its [q blocks, max_blocks] table
//          exist.
//          Causality is exploited, not only masked.  With lim(t) = min(L, pos(t) + 1) the keys visible to token t: blocks at or behind
//          ceil(max_t lim / bs) are neither looked up nor loaded (the tile writes their -inf), K rows at or behind max_t lim are zeros that
//          are never read, blocks that end at or below min_t lim take no per-row mask, and only the blocks between compare per row.
//          Workgroup order: tile fastest, then run, then kv head -- the workgroups resident at one time are the tiles of one request against
//          the SAME run of keys (2048 keys: 512 KB at head dim 128), which they share through L2.
//  select  one wave per (head, token) row, four rows per workgroup, no workgroup barrier.  Every block has the distinct 46-bit key
//          (descending-order image of its score) << 14 | j (block_key, shared with the decode form); k = min(topk, scores above -inf); the
//          k-th smallest key is found by bisection on the key's bits (ballots; the keys of rows of up to 512 blocks stay in registers, longer
//          rows are re-read), the k winners are compacted into the wave's own LDS slice and each finds its rank by counting.  Fused form:
//          entries that start behind the token's position become -1 in place and slot topk receives the causal-local block.
//
// LIMITS (refused with MI_SGL_EINVAL, never a silent wrong answer): max_seqblock <= 16384; topk <= 1024; block_size 16 / 32 / 64 / 128;
// head_dim a multiple of 8 up to 256 (padded with zeros to 64 / 128 / 256); sm_scale > 0.
#include <algorithm>

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_score_dev.h"
#include "mi_sgl_kernels.h"

namespace mi_gqa_prefill_score {
using namespace mi_gqa;

constexpr int kColBlocks = 4, kTileRows = 16 * kColBlocks;       // rows (token, head) of a workgroup
constexpr int kRunKeys = 2048;                                   // keys of a run of blocks
constexpr int kSelRegIters = 8;                                  // select: rows of up to 64 * 8 blocks keep their keys in registers

struct Params {
    const uint16_t *q, *k;
    float *score;                   // [heads, total_q, max_seqblock]
    const void *cu, *seq_lens, *qpos;
    int cu_i64, sl_i64, qpos_i64;
    PageMap pages;                  // always the req_to_token form
    int total_q, nreq, heads, kv_heads, group, gc, tq, head_blocks, block_size, bs_shift, max_seqblock, d;
    int tiles, runs, blocks_per_wg;
    int64_t q_st, q_sh, k_sblk, k_srow, k_sh, s_sh, s_st;
    float sm_scale;
};

// DP: compile-time padded head dim (64, 128, 256)
template <bool BF16, int DP, bool LSE>
__global__ __launch_bounds__(256) void gqa_prefill_block_score_kernel(Params p)
{
    constexpr int CB = kColBlocks, QS = DP / 32;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    int u = blockIdx.x;                                           // the grid is exactly tiles * runs * kv_heads * head_blocks
    int tile = u % p.tiles;
    u /= p.tiles;
    const int run = u % p.runs;
    u /= p.runs;
    const int hblk = u % p.head_blocks, kvh = u / p.head_blocks;
    const int BS = p.block_size, shift = p.bs_shift;

    // the tile's request: tiles are dealt request by request, ceil(q_len / TQ) each; what is left covers the tokens behind cu[nreq]
    int req = -1;
    int64_t t0 = 0, tend = 0, cu0 = 0, q_len = 0;
    {
        int64_t lo = load_index(p.cu, p.cu_i64, 0);
        for (int r = 0; r < p.nreq; ++r) {
            const int64_t hi = load_index(p.cu, p.cu_i64, r + 1);
            const int64_t nt = hi > lo ? (hi - lo + p.tq - 1) / p.tq : 0;
            if (tile < nt) {
                req = r, cu0 = lo, q_len = hi - lo, t0 = lo + (int64_t)tile * p.tq, tend = hi;
                break;
            }
            tile -= (int)nt;
            lo = hi;
        }
        if (req < 0) t0 = max(lo, (int64_t)0) + (int64_t)tile * p.tq, tend = p.total_q;
    }
    tend = min(tend, (int64_t)p.total_q);
    if (t0 < 0 || t0 >= tend) return;                             // wave-uniform: a tile the bound holds in reserve
    const int ntok = (int)min(tend - t0, (int64_t)p.tq);

    // keys visible to token t: positions below lim(t) = min(L, pos(t) + 1); 0 for the tokens no request owns and for a negative position
    int L = 0;
    int64_t pos_base = 0;                                         // true position of token cu0
    int64_t pool_row = 0;
    if (req >= 0) {
        const int64_t sl = load_index(p.seq_lens, p.sl_i64, req);
        L = (int)min(max(sl, (int64_t)0), (int64_t)p.max_seqblock * BS);
        pos_base = sl - q_len;
        pool_row = load_index(p.pages.req_pool, p.pages.req_i64, req);
    }
    auto lim_of = [&](int64_t t) -> int {
        if (req < 0) return 0;
        const int64_t pos = p.qpos ? load_index(p.qpos, p.qpos_i64, t) : pos_base + (t - cu0);
        return pos < 0 ? 0 : (int)min((int64_t)L, pos + 1);
    };
    int lim_lo = lane < ntok ? lim_of(t0 + lane) : 0x7fffffff, lim_hi = lane < ntok ? lim_of(t0 + lane) : 0;      // TQ <= 64 tokens
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lim_lo = min(lim_lo, __shfl_xor(lim_lo, o));
        lim_hi = max(lim_hi, __shfl_xor(lim_hi, o));
    }
    const int lim_min = __builtin_amdgcn_readfirstlane(lim_lo), lim_max = __builtin_amdgcn_readfirstlane(lim_hi);
    const int nb_tile = (lim_max + BS - 1) >> shift;              // blocks at or behind it hold no visible key for any row of the tile

    const int jrun0 = run * p.blocks_per_wg, jrun1 = min(jrun0 + p.blocks_per_wg, p.max_seqblock);
    const int jw = jrun0 + wave;                                  // this wave's blocks: jw, jw + 4, ... below j1
    const int j1 = min(jrun1, nb_tile);

    if (jw < j1) {                                                // no LDS, no barrier: waves are on their own
        // Q^T fragments: lane (g, c16) holds q[token][head][ks*32 + g*8 .. +8] of row cb * 16 + c16 = (token, head) token-major; its lim
        s16x8 qf[CB][QS];
        int lim_row[CB];
        int64_t srow[CB];                                         // offset of the row's scores; -1 = no such row
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            const int r = cb * 16 + c16, ti = r / p.gc, hg = hblk * kTileRows + r % p.gc;
            const bool ok = ti < ntok && hg < p.group;
            const int head = kvh * p.group + hg;
            const int64_t t = t0 + (ok ? ti : 0);
            lim_row[cb] = ok ? lim_of(t) : 0;
            srow[cb] = ok ? (int64_t)head * p.s_sh + t * p.s_st : -1;
            const uint16_t *qrow = p.q + t * p.q_st + (int64_t)(ok ? head : 0) * p.q_sh;
#pragma unroll
            for (int ks = 0; ks < QS; ++ks) {
                const int d = ks * 32 + g * 8;
                qf[cb][ks] = (ok && d < p.d) ? *(const s16x8 *)(qrow + d) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
        // jl < j1 <= nb_tile <= ceil(L / BS); rows no row of the tile sees are zeros and are never read; blocks every row sees whole skip the mask
        score_blocks<BF16, DP, CB, LSE>(
            KeyRows{p.k + (int64_t)kvh * p.k_sh, p.k_sblk, p.k_srow, p.d, BS, shift}, jw, j1, qf, lim_row, lim_max, lim_min,
            p.sm_scale * 1.4426950408889634f, [&](int j) { return page_of_row(p.pages, pool_row, j, BS); },
            [&](int cb, int j, float score) {
                if (srow[cb] >= 0) p.score[srow[cb] + j] = score;
            });
    }

    // the run's blocks at or behind nb_tile: -inf for every row of the tile (wave w: rows w, w + 4, ...; lanes along the blocks)
    const int jf0 = max(jrun0, nb_tile);
    if (jf0 < jrun1) {
        const int rows = ntok * p.gc;
        for (int r = wave; r < rows; r += 4) {
            const int ti = r / p.gc, hg = hblk * kTileRows + r % p.gc;
            if (hg >= p.group) continue;
            float *dst = p.score + (int64_t)(kvh * p.group + hg) * p.s_sh + (t0 + ti) * p.s_st;
            for (int j = jf0 + lane; j < jrun1; j += 64) dst[j] = -INFINITY;
        }
    }
}

struct SelParams {
    const float *score;
    int64_t s_sh, s_st, s_sk;
    const void *lens;               // [total_q] causal length of every token (fused form)
    int lens_i64;
    int32_t *out;                   // [heads, total_q, topk (+ 1 fused)]
    int heads, total_q, max_seqblock, topk, block_size, fused;
};

// one wave per row; REG: max_seqblock <= 64 * kSelRegIters, the row's keys stay in registers.  LDS: the wave's winners (8 B x topk).
template <bool REG>
__global__ __launch_bounds__(256) void prefill_block_select_kernel(SelParams p)
{
    __shared__ uint64_t win_all[4][kMaxTopk];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= (int64_t)p.heads * p.total_q) return;              // wave-uniform; no workgroup barrier below
    const int h = (int)(row / p.total_q), t = (int)(row % p.total_q);
    const int nblk = p.max_seqblock, iters = (nblk + 63) >> 6;
    const float *srow = p.score + (int64_t)h * p.s_sh + (int64_t)t * p.s_st;
    int32_t *orow = p.out + row * (p.topk + (p.fused ? 1 : 0));
    uint64_t *win = win_all[wave];

    auto key_at = [&](int i) -> uint64_t {                        // padding lanes: a key above every real one
        const int j = i * 64 + lane;
        return j < nblk ? block_key(srow[(int64_t)j * p.s_sk], j) : ~0ull;
    };
    uint64_t kreg[kSelRegIters];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < kSelRegIters; ++i) kreg[i] = i < iters ? key_at(i) : ~0ull;
    }
    auto count_le = [&](uint64_t c) -> int {                      // keys at or below c (the same in every lane)
        int n = 0;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kSelRegIters; ++i) n += __popcll(__ballot(kreg[i] <= c));
        } else {
            for (int i = 0; i < iters; ++i) n += __popcll(__ballot(key_at(i) <= c));
        }
        return n;
    };
    const uint64_t below_inf = block_key(-INFINITY, 0) - 1;      // every score above -inf has a key at or below it
    const int nfin = count_le(below_inf);
    const int k = min(p.topk, nfin);
    uint64_t T = below_inf;
    if (nfin > p.topk) {                                          // the k-th smallest key, bit by bit from the top
        T = 0;
        for (int bit = 31 + kIdxBits; bit >= 0; --bit)
            if (count_le(T | ((1ull << bit) - 1)) < k) T |= 1ull << bit;
    }
    // the k winners (keys are distinct: exactly k lie at or below T) in block order into the wave's LDS slice
    int base = 0;
    auto compact = [&](uint64_t key) {
        const bool in = key <= T;
        const uint64_t b = __ballot(in);
        if (in) win[base + __popcll(b & ((1ull << lane) - 1))] = key;
        base += __popcll(b);
    };
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < kSelRegIters; ++i) compact(kreg[i]);
    } else {
        for (int i = 0; i < iters; ++i) compact(key_at(i));
    }
    __builtin_amdgcn_wave_barrier();                              // LDS operations of one wave complete in order
    int64_t qpos = 0;
    int local = -2;
    if (p.fused) {
        qpos = max(load_index(p.lens, p.lens_i64, t) - 1, (int64_t)0);
        local = (int)min(qpos / p.block_size, (int64_t)nblk - 1);
    }
    bool hit = false;
    for (int w = lane; w < k; w += 64) {                          // rank = winners with a smaller key
        const uint64_t mine = win[w];
        int rank = 0;
        for (int x = 0; x < k; ++x) rank += win[x] < mine;
        int v = (int)(mine & (kMaxSeqBlock - 1));
        if (p.fused && (int64_t)v * p.block_size > qpos) v = -1;
        orow[rank] = v;
        hit |= v == local;
    }
    for (int s = k + lane; s < p.topk; s += 64) orow[s] = -1;
    const bool any = __any(hit);
    if (p.fused && lane == 0) orow[p.topk] = any ? -1 : local;
}

}  // namespace mi_gqa_prefill_score

using namespace mi_gqa_prefill_score;

extern "C" int mi_gqa_prefill_block_score(const void *q, const void *k, float *score, const void *cu_seqlens, int cu_seqlens_is_i64,
                                          const void *seq_lens, int seq_lens_is_i64, const void *req_to_token, int req_to_token_is_i64,
                                          int64_t rtt_stride_r, int64_t rtt_stride_t, int rtt_cols, const void *req_pool_indices,
                                          int req_pool_is_i64, const void *query_pos, int query_pos_is_i64, int total_q, int num_reqs,
                                          int idx_heads, int kv_heads, int head_dim, int block_size, int max_seqblock, int score_lse,
                                          int64_t q_stride_t, int64_t q_stride_h, int64_t k_stride_blk, int64_t k_stride_row, int64_t k_stride_h,
                                          int64_t s_stride_h, int64_t s_stride_t, float sm_scale, int dtype, void *stream)
{
    if (total_q < 0 || num_reqs < 0 || idx_heads <= 0 || kv_heads <= 0 || idx_heads % kv_heads) return MI_SGL_EINVAL;
    if (!block_args_ok(block_size, head_dim, dtype, sm_scale)) return MI_SGL_EINVAL;
    if (max_seqblock <= 0 || max_seqblock > kMaxSeqBlock || rtt_cols <= 0) return MI_SGL_EINVAL;      // the declared limits
    if (total_q == 0) return MI_SGL_OK;
    if (!q || !k || !score || !cu_seqlens) return MI_SGL_EINVAL;
    if (num_reqs > 0 && (!seq_lens || !req_to_token || !req_pool_indices)) return MI_SGL_EINVAL;
    if (!aligned8({q_stride_h, q_stride_t, k_stride_row, k_stride_blk, k_stride_h})) return MI_SGL_EINVAL;
    Params p;
    p.q = (const uint16_t *)q, p.k = (const uint16_t *)k, p.score = score;
    p.cu = cu_seqlens, p.seq_lens = seq_lens, p.qpos = query_pos;
    p.cu_i64 = cu_seqlens_is_i64, p.sl_i64 = seq_lens_is_i64, p.qpos_i64 = query_pos_is_i64;
    p.pages = make_page_map(nullptr, 0, 0, 0, req_to_token, req_to_token_is_i64, rtt_stride_r, rtt_stride_t, rtt_cols, req_pool_indices,
                            req_pool_is_i64, 0, 0);
    p.total_q = total_q, p.nreq = num_reqs, p.heads = idx_heads, p.kv_heads = kv_heads, p.group = idx_heads / kv_heads;
    // the tile: TQ tokens x gc heads <= 64 rows, token-major; groups above 64 heads take one token and several head blocks
    p.gc = std::min(p.group, kTileRows);
    p.tq = kTileRows / p.gc;
    p.head_blocks = (p.group + kTileRows - 1) / kTileRows;
    p.block_size = block_size, p.bs_shift = __builtin_ctz(block_size), p.max_seqblock = max_seqblock, p.d = head_dim;
    p.tiles = (total_q + p.tq - 1) / p.tq + num_reqs;             // >= sum of ceil(q_len / TQ) over the requests and the tokens behind them
    p.blocks_per_wg = std::max(4, kRunKeys / block_size);         // a multiple of the four waves
    p.runs = (max_seqblock + p.blocks_per_wg - 1) / p.blocks_per_wg;
    p.q_st = q_stride_t, p.q_sh = q_stride_h, p.k_sblk = k_stride_blk, p.k_srow = k_stride_row, p.k_sh = k_stride_h;
    p.s_sh = s_stride_h, p.s_st = s_stride_t;
    p.sm_scale = sm_scale;
    const long long wgs = (long long)p.tiles * p.runs * kv_heads * p.head_blocks;
    if (wgs > 0x7fffffffll) return MI_SGL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    dispatch(dtype == MI_DTYPE_BF16, padded_dim(head_dim), score_lse != 0, [&](auto bf, auto dp, auto lse) {
        gqa_prefill_block_score_kernel<bf(), dp(), lse()><<<(unsigned)wgs, 256, 0, st>>>(p);
    });
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}

extern "C" int mi_prefill_topk_from_score(const float *score, int64_t s_stride_h, int64_t s_stride_t, int64_t s_stride_k,
                                          const void *per_query_seq_lens, int per_query_seq_lens_is_i64, int32_t *topk_idx, int heads,
                                          int total_q, int max_seqblock, int topk, int block_size, int fused, void *stream)
{
    if (heads < 0 || total_q < 0 || block_size <= 0) return MI_SGL_EINVAL;
    if (!within_limits(max_seqblock, topk)) return MI_SGL_EINVAL; // the declared limits
    if (fused && !per_query_seq_lens) return MI_SGL_EINVAL;
    const int64_t rows = (int64_t)heads * total_q;
    if (rows == 0) return MI_SGL_OK;
    if (!score || !topk_idx || (rows + 3) / 4 > 0x7fffffffll) return MI_SGL_EINVAL;
    SelParams p;
    p.score = score, p.s_sh = s_stride_h, p.s_st = s_stride_t, p.s_sk = s_stride_k;
    p.lens = per_query_seq_lens, p.lens_i64 = per_query_seq_lens_is_i64, p.out = topk_idx;
    p.heads = heads, p.total_q = total_q, p.max_seqblock = max_seqblock, p.topk = topk, p.block_size = block_size, p.fused = fused != 0;
    const unsigned grid = (unsigned)((rows + 3) / 4);
    if (max_seqblock <= 64 * kSelRegIters) prefill_block_select_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    else prefill_block_select_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}
