// Block-score indexer of the block-sparse GQA decode for gfx950: which KV blocks should a sequence attend to?  Replaces the score-only form of
// the reference's Triton-Ascend `flash_decode_bnsd_with_topk_idx` (python/sgl_kernel_npu/sgl_kernel_npu/indexer/flash_block_score_decode.py:
// 749-1029 score + per-chunk top-k, :97-420 candidate merge, :426-527 merge with the causal-local append, :1451-1562 the standalone append).
// Produces the topk_idx [Hq, B, topk] that gqa_sparse_decode.hip consumes.
//
// Two stream-ordered launches, both sized from host integers (shapes, max_seqblock) only -- nothing is read back, the op replays in a graph:
//
//  score   a workgroup of 4 waves owns (sequence, kv head, block of query heads, run of logical KV blocks); wave w takes the run's blocks
//          w, w + 4, ... through score_blocks of block_score_dev.h, the engine the prefill form (gqa_block_score_prefill.hip) runs too.
//          There is no V, no P.V, no accumulator and no LDS: a wave loads 16 keys x head_dim of its block straight into the
//          A operand of mfma_f32_16x16x32 (lane (g, c16): key c16, dims ks*32 + 8g .. +8 -- every K byte is loaded once, by one lane),
//          S^T = K.Q^T against the Q^T fragments of all heads of the group it keeps in registers, so every K byte leaves HBM once per kv
//          head.  Keys are masked by logical position against the row's own length; the per-block maximum (and, for "lse", the exp2 sum,
//          kept online per lane) is fp32 in the log2 domain; the four lane rows meet in permlane swaps when a block ends.  Loads run one
//          stage (64 keys, 32 at head dims above 128) ahead of the MFMAs in a second register set.  Rows at or behind the group's longest
//          length are not loaded (zeros), table entries of blocks that start there are not read.  Scores go to an fp32 workspace
//          [B, Hq, max_seqblock].
//  select  a workgroup per (sequence, query head): the row's scores, forced values applied (block j < init_blocks: 1e30; then
//          j >= max(0, nb - local_blocks): 1e29), sit in LDS (4 B x max_seqblock <= 64 KB).  Every block has the distinct 46-bit key
//          (descending-order image of its score) << 14 | j; the k-th smallest key, k = min(topk, nb), is found by bisection on the key's
//          bits (46 counting passes, one barrier each), the k keys at or below it are compacted and sorted (bitonic, <= 1024 entries) and
//          written: descending score, ties by ascending block id, -1 behind them.  Optionally slot topk receives the causal-local block.
//          When the group's largest block count is <= topk nothing was scored and the row is 0 .. nb - 1.
//
// LIMITS (refused with MI_SGL_EINVAL, never a silent wrong answer): max_seqblock <= 16384; topk <= 1024; block_size 16 / 32 / 64 / 128;
// head_dim a multiple of 8 up to 256 (padded with zeros to 64 / 128 / 256); sm_scale > 0 (the scaling is applied before the maximum, but
// forced values and -inf are not scaled).  Lengths are clamped to [0, min(max_seqblock, table columns) * block_size].
#include <algorithm>

#include "device_once.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_score_dev.h"
#include "mi_sgl_kernels.h"

namespace mi_gqa_score {
using namespace mi_gqa;

struct Params {
    const uint16_t *q, *k;
    const int32_t *seq_lens;        // [batch] (sl_sb = 1, sl_sh = 0) or, packed, [batch * group] (sl_sb = group, sl_sh = 1)
    int sl_sb, sl_sh;
    PageMap pages;
    float *scores;                  // [batch, q_heads, max_seqblock]
    int32_t *out;                   // [q_heads, batch, topk (+ 1 with append_blocks > 0)]
    int batch, q_heads, kv_heads, group, block_size, bs_shift, max_seqblock, max_kv_len, topk, init_blocks, local_blocks, lse, append_blocks, d;
    int runs, blocks_per_wg, head_blocks;
    int64_t q_sb, q_sh, k_sblk, k_srow, k_sh;
    float sm_scale;
};

__device__ __forceinline__ int row_len(const Params &p, int b, int hg)
{
    return min(max(p.seq_lens[(int64_t)b * p.sl_sb + (int64_t)hg * p.sl_sh], 0), p.max_kv_len);
}
__device__ __forceinline__ int group_max_len(const Params &p, int b)      // the same in every thread
{
    int len = row_len(p, b, 0);
    if (p.sl_sh)
        for (int i = 1; i < p.group; ++i) len = max(len, row_len(p, b, i));
    return len;
}

// DP: compile-time padded head dim (64, 128, 256); HB: blocks of 16 query heads a workgroup covers (every wave holds all of them).
template <bool BF16, int DP, int HB, bool LSE>
__global__ __launch_bounds__(256) void gqa_block_score_kernel(Params p)
{
    constexpr int QS = DP / 32;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    int u = blockIdx.x;                                           // the grid is exactly batch * kv_heads * runs * head_blocks
    const int hblk = u % p.head_blocks;
    u /= p.head_blocks;
    const int run = u % p.runs;
    u /= p.runs;
    const int kvh = u % p.kv_heads, b = u / p.kv_heads;
    const int BS = p.block_size, shift = p.bs_shift;

    const int len_max = group_max_len(p, b);
    const int nb_max = (len_max + BS - 1) >> shift;
    if (nb_max <= p.topk) return;                                 // nothing is scored: the select launch writes 0 .. nb - 1
    const int jw = run * p.blocks_per_wg + wave;                  // this wave's blocks: jw, jw + 4, ... below j1
    const int j1 = min((run + 1) * p.blocks_per_wg, nb_max);
    if (jw >= j1) return;                                         // no LDS, no barrier: waves are on their own

    // Q^T fragments: lane (g, c16) holds q[head][ks*32 + g*8 .. +8] of head block hb; its row's length
    s16x8 qf[HB][QS];
    int head[HB], len_row[HB];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        const int hg = (hblk * HB + hb) * 16 + c16;
        const bool ok = hg < p.group;
        head[hb] = ok ? kvh * p.group + hg : -1;
        len_row[hb] = ok ? row_len(p, b, hg) : 0;
        const uint16_t *qrow = p.q + (int64_t)b * p.q_sb + (int64_t)(ok ? head[hb] : 0) * p.q_sh;
#pragma unroll
        for (int ks = 0; ks < QS; ++ks) {
            const int d = ks * 32 + g * 8;
            qf[hb][ks] = (ok && d < p.d) ? *(const s16x8 *)(qrow + d) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    // every block takes the per-row mask (lim_min 0); rows at or behind the group's longest length are zeros and are never read
    score_blocks<BF16, DP, HB, LSE>(
        KeyRows{p.k + (int64_t)kvh * p.k_sh, p.k_sblk, p.k_srow, p.d, BS, shift}, jw, j1, qf, len_row, len_max, 0, p.sm_scale * 1.4426950408889634f,
        [&](int j) { return page_of(p.pages, b, j, BS); },
        [&](int hb, int j, float score) {
            if (head[hb] >= 0) p.scores[((int64_t)b * p.q_heads + head[hb]) * p.max_seqblock + j] = score;
        });
}

// one workgroup per (sequence, query head); P = power of two >= max(2, topk); LDS: P keys (8 B), max_seqblock scores (4 B), 16 words
__global__ __launch_bounds__(256) void gqa_block_select_kernel(Params p, int P, int sc_words)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t *cand = (uint64_t *)lds;
    float *sc = (float *)(lds + 8 * (size_t)P);
    int *cnt = (int *)(sc + sc_words);                            // [0..7] two sets of per-wave counts, [8] compaction cursor, [9] local block seen
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x % p.q_heads, b = blockIdx.x / p.q_heads;
    const int BS = p.block_size, shift = p.bs_shift;
    const int len = row_len(p, b, h % p.group);
    const int nb = (len + BS - 1) >> shift;
    const int nb_max = (group_max_len(p, b) + BS - 1) >> shift;
    const bool append = p.append_blocks > 0;
    const int local = append ? min(max(len - 1, 0) >> shift, p.append_blocks - 1) : -2;
    int32_t *orow = p.out + ((int64_t)h * p.batch + b) * (p.topk + (append ? 1 : 0));
    // an entry the append form does not let through (the standalone append kernel's check; every entry here is below nb already)
    auto checked = [&](int v) { return (append && v >= p.append_blocks) ? -1 : v; };

    if (nb_max <= p.topk) {                                       // wave-uniform: nothing was scored
        for (int t = tid; t < p.topk; t += 256) orow[t] = t < nb ? checked(t) : -1;
        if (append && tid == 0) orow[p.topk] = local < nb ? -1 : local;
        return;
    }
    const int k = min(p.topk, nb);
    const int local_start = p.local_blocks > 0 ? max(0, nb - p.local_blocks) : nb;
    const float *srow = p.scores + ((int64_t)b * p.q_heads + h) * p.max_seqblock;
    for (int j = tid; j < nb; j += 256) {
        float s = srow[j];
        if (j < p.init_blocks) s = 1e30f;
        if (j >= local_start) s = 1e29f;
        sc[j] = s;
    }
    if (tid < 16) cnt[tid] = 0;
    __syncthreads();

    // the k-th smallest key, bit by bit from the top: a bit stays 0 when k keys lie at or below (prefix | all lower bits set)
    uint64_t T = 0;
    for (int bit = 31 + kIdxBits, it = 0; bit >= 0; --bit, ++it) {
        const uint64_t c = T | ((1ull << bit) - 1);
        int n = 0;
        for (int base = wave * 64; base < nb; base += 256) {
            const int j = base + lane;
            n += __popcll(__ballot(j < nb && block_key(sc[min(j, nb - 1)], j) <= c));
        }
        int *slot = cnt + (it & 1) * 4;                           // two sets: a wave two passes ahead cannot exist (one barrier per pass)
        if (lane == 0) slot[wave] = n;
        __syncthreads();
        if (slot[0] + slot[1] + slot[2] + slot[3] < k) T |= 1ull << bit;
    }
    // the k winners (keys are distinct: exactly k lie at or below T), compacted in any order, padded, sorted
    for (int j = tid; j < nb; j += 256) {
        const uint64_t key = block_key(sc[j], j);
        if (key <= T) cand[atomicAdd(&cnt[8], 1)] = key;
    }
    for (int t = k + tid; t < P; t += 256) cand[t] = ~0ull;
    __syncthreads();
    bitonic_sort<256>(cand, P);
    for (int t = tid; t < p.topk; t += 256) {
        const int v = t < k ? checked((int)(cand[t] & (kMaxSeqBlock - 1))) : -1;
        orow[t] = v;
        if (v == local) cnt[9] = 1;
    }
    if (append) {
        __syncthreads();
        if (tid == 0) orow[p.topk] = cnt[9] ? -1 : local;
    }
}

// [heads, batch, topk] -> [heads, batch, topk + 1]; one wave per row
__global__ __launch_bounds__(256) void topk_append_local_kernel(const int32_t *in, const int32_t *seq_lens, int32_t *out, int64_t rows, int batch, int topk,
                                                                int block_size, int num_blocks)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int qpos = max(seq_lens[row % batch] - 1, 0);
    const int local = min(qpos / block_size, num_blocks - 1);
    bool hit = false;
    for (int t = lane; t < topk; t += 64) {
        int v = in[row * topk + t];
        if (v < 0 || v >= num_blocks || (int64_t)v * block_size > qpos) v = -1;
        out[row * (topk + 1) + t] = v;
        hit |= v == local;
    }
    const bool any = __any(hit);
    if (lane == 0) out[row * (topk + 1) + topk] = any ? -1 : local;
}

}  // namespace mi_gqa_score

using namespace mi_gqa_score;

extern "C" size_t mi_gqa_block_score_topk_workspace(int batch, int q_heads, int max_seqblock)
{
    if (batch <= 0 || q_heads <= 0 || max_seqblock <= 0 || max_seqblock > kMaxSeqBlock) return 0;
    return (size_t)batch * q_heads * max_seqblock * sizeof(float);
}

extern "C" int mi_gqa_block_score_topk(const void *q, const void *k, int32_t *topk_idx, const int32_t *seq_lens, int packed_seq_lens,
                                       const void *block_table, int block_table_is_i64, int64_t bt_stride_b, int64_t bt_stride_n, int bt_cols,
                                       const void *req_to_token, int req_to_token_is_i64, int64_t rtt_stride_r, int64_t rtt_stride_t,
                                       int rtt_cols, const void *req_pool_indices, int req_pool_is_i64, int batch, int q_heads, int kv_heads,
                                       int head_dim, int block_size, int max_seqblock, int topk, int init_blocks, int local_blocks,
                                       int score_lse, int append_local_num_blocks, int num_pages, int sanitize_page_ids, int64_t q_stride_b,
                                       int64_t q_stride_h, int64_t k_stride_blk, int64_t k_stride_row, int64_t k_stride_h, float sm_scale,
                                       int dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    if (batch < 0 || q_heads <= 0 || kv_heads <= 0 || q_heads % kv_heads) return MI_SGL_EINVAL;
    if (!block_args_ok(block_size, head_dim, dtype, sm_scale)) return MI_SGL_EINVAL;
    if (!within_limits(max_seqblock, topk)) return MI_SGL_EINVAL; // the declared limits
    if (init_blocks < 0 || local_blocks < 0 || append_local_num_blocks < 0) return MI_SGL_EINVAL;
    const bool direct = req_to_token != nullptr;
    if (direct == (block_table != nullptr) || direct != (req_pool_indices != nullptr)) return MI_SGL_EINVAL;
    if (direct ? (rtt_cols <= 0 || num_pages <= 0) : bt_cols <= 0) return MI_SGL_EINVAL;
    if (batch == 0) return MI_SGL_OK;
    if (!q || !k || !topk_idx || !seq_lens) return MI_SGL_EINVAL;
    if (!aligned8({q_stride_h, q_stride_b, k_stride_row, k_stride_blk, k_stride_h})) return MI_SGL_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < mi_gqa_block_score_topk_workspace(batch, q_heads, max_seqblock))
        return MI_SGL_EINVAL;
    Params p;
    p.q = (const uint16_t *)q, p.k = (const uint16_t *)k, p.seq_lens = seq_lens;
    p.group = q_heads / kv_heads;
    p.sl_sb = packed_seq_lens ? p.group : 1, p.sl_sh = packed_seq_lens ? 1 : 0;
    p.pages = make_page_map(block_table, block_table_is_i64, bt_stride_b, bt_stride_n, req_to_token, req_to_token_is_i64, rtt_stride_r,
                            rtt_stride_t, rtt_cols, req_pool_indices, req_pool_is_i64, num_pages, sanitize_page_ids);
    p.scores = (float *)workspace, p.out = topk_idx;
    p.batch = batch, p.q_heads = q_heads, p.kv_heads = kv_heads, p.block_size = block_size, p.bs_shift = __builtin_ctz(block_size);
    p.max_seqblock = max_seqblock;
    p.max_kv_len = (direct ? max_seqblock : std::min(max_seqblock, bt_cols)) * block_size;      // <= 16384 * 128
    p.topk = topk, p.init_blocks = init_blocks, p.local_blocks = local_blocks, p.lse = score_lse != 0;
    p.append_blocks = append_local_num_blocks, p.d = head_dim;
    p.q_sb = q_stride_b, p.q_sh = q_stride_h, p.k_sblk = k_stride_blk, p.k_srow = k_stride_row, p.k_sh = k_stride_h;
    p.sm_scale = sm_scale;
    // head blocks of 16 (one MFMA column block) or 64 heads; runs of logical blocks: about eight workgroups per CU, a wave with at least
    // 128 keys, a multiple of the four waves
    const int hb = p.group <= 16 ? 1 : 4;
    p.head_blocks = (p.group + 16 * hb - 1) / (16 * hb);
    const long long cells = (long long)batch * kv_heads * p.head_blocks;
    const int min_bpw = 4 * std::max(1, 128 / block_size);
    long long runs = std::min<long long>((8ll * cus() + cells - 1) / cells, (max_seqblock + min_bpw - 1) / min_bpw);
    runs = std::max<long long>(runs, 1);
    p.blocks_per_wg = (int)(((max_seqblock + runs - 1) / runs + 3) / 4 * 4);
    p.runs = (max_seqblock + p.blocks_per_wg - 1) / p.blocks_per_wg;
    const long long wgs = cells * p.runs;
    if (wgs > 0x7fffffffll || (long long)batch * q_heads > 0x7fffffffll) return MI_SGL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (max_seqblock > topk)                                      // otherwise no sequence can hold more than topk blocks: select alone
        dispatch(dtype == MI_DTYPE_BF16, padded_dim(head_dim), p.lse, [&](auto bf, auto dp, auto lse) {
            if (hb == 1) gqa_block_score_kernel<bf(), dp(), 1, lse()><<<(unsigned)wgs, 256, 0, st>>>(p);
            else gqa_block_score_kernel<bf(), dp(), 4, lse()><<<(unsigned)wgs, 256, 0, st>>>(p);
        });
    int P = 2;
    while (P < topk) P *= 2;
    const int sc_words = (max_seqblock + 3) / 4 * 4;
    const size_t lds = 8 * (size_t)P + 4 * (size_t)sc_words + 64;
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        (void)hipFuncSetAttribute((const void *)gqa_block_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(8 * kMaxTopk + 4 * kMaxSeqBlock + 64));
    gqa_block_select_kernel<<<(unsigned)(batch * q_heads), 256, lds, st>>>(p, P, sc_words);
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}

extern "C" int mi_topk_append_local_block(const int32_t *topk_idx, const int32_t *seq_lens, int32_t *out, int heads, int batch, int topk,
                                          int block_size, int num_blocks, void *stream)
{
    if (heads < 0 || batch < 0 || topk < 0 || block_size <= 0 || num_blocks <= 0) return MI_SGL_EINVAL;
    const int64_t rows = (int64_t)heads * batch;
    if (rows == 0) return MI_SGL_OK;
    if (!seq_lens || !out || (topk > 0 && !topk_idx) || (rows + 3) / 4 > 0x7fffffffll) return MI_SGL_EINVAL;
    topk_append_local_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(topk_idx, seq_lens, out, rows, batch, topk, block_size,
                                                                                        num_blocks);
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}
