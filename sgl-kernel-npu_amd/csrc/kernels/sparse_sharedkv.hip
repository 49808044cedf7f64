// sparse_attn_sharedkv for gfx950 (MI355X), bf16 / fp16: 64-head MQA over ONE shared 512-wide latent that is both K and V; a query token
// attends to a sliding window over the original cache plus, optionally, a compressed cache that is read whole (up to its causal limit) or at
// the key indices an indexer chose (the consumer of lightning_indexer.hip).  A per-head sink logit sits in the softmax denominator.
// Replaces the reference's AscendC op csrc/sparse_attn_sharedkv/ (op_kernel/arch32/sparse_attn_sharedkv_{swa,scfa}_kernel.h); the semantics
// are stated in include/mi_sgl_kernels.h and DESIGN.md 4.3.6.
//
// Schedule: the 64-heads-per-workgroup form of mla_decode.hip without the rope part; the tile engine both share (fill primitive, QK pipeline,
// softmax step, P.V, the two finishes) is latent_tile_dev.h.  This file holds the op's own: the key list and its three-step addressing, the
// mask from the tile's ballot, the tile skip, the sink start values and the merge.
//  * one workgroup = one query token x one piece of its key list; 4 waves, one per SIMD, 16 heads each (lane = head for the softmax
//    statistics), all 512 output dims per wave (128 accumulators + 64 resident Q^T registers);
//  * the key list of a token is its window keys followed by its index slots (or by the `limit` compressed keys).  Lane l of a tile owns list
//    position 64 t + l and turns it into the absolute address of one 1-KiB row: window position -> ori_block_table -> ori_kv, slot -> index
//    -> cmp_block_table -> cmp_kv (64-bit offsets), in three steps that run one tile apart (index of tile t + 3, table entry of tile t + 2,
//    address + fill of tile t + 1 under the MFMAs of tile t) so no load is waited for where it is issued;
//  * tiles of 64 rows go global -> LDS by LDS-DMA (one row per wave-instruction, issued one per QK k-step: 16 rows per wave = 16 k-steps),
//    double buffered (2 x 66 KB), one barrier per tile; rows padded to 1056 B as in mla_decode.hip;
//  * a position that does not count (slot < 0 or >= limit, or behind the list) is masked to -inf in S and its row address is the token's own
//    newest window key: the caches may hold anything (NaN) in rows the token must not read, and 0 * NaN would reach O through P.V.  A tile
//    without a counting position is neither filled nor computed (wave-uniform test on the tile's ballot), wherever it stands;
//  * online softmax in the engine's whole-number-reference form (softmax_step<., true>); piece 0 starts from the sink, (m, l) = (ceil(sink),
//    2^(sink - m)) -- the (sink, 1) of the semantics --, the others from (-inf, 0); with one piece the kernel writes the output, otherwise a
//    merge kernel combines the fp32 (m, l, O) partials.
// Algorithmic HBM bytes per call: sum over tokens of (counting keys) * 1024 + tokens * 64 * 512 * 2 * 2 (Q, out).
#include "device_once.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mi_sgl_kernels.h"
#include "gqa_common.h"      // cus()
#include "latent_tile_dev.h"

namespace mi_sgl {
namespace {

constexpr int kHeads = 64;
constexpr int kSskBuf = kTile * kNopeStride;      // 67584 B per tile
constexpr int kMaxSplits = 64;
constexpr int kMaxSparse = 2048;

struct SskParams {
    const uint16_t *q, *ori_kv, *cmp_kv;
    uint16_t *out;
    const float *sinks;
    const int32_t *idx, *ori_bt, *cmp_bt, *cu_q, *seqused_q, *seqused_kv;
    float *ws_o, *ws_ml;      // [tokens][64][num_splits][512] / [..][2] fp32 partials
    int tnd, batch, s1, num_splits;
    int64_t tokens;
    int ori_block, cmp_block, ori_cap, cmp_cap, sparse_k, cmp_ratio, win_left, win_right;
    int64_t q_sb, q_ss, q_sh, o_sb, o_ss, o_sh, idx_sb, idx_ss;
    int64_t ori_sblk, cmp_sblk, ori_bt_sb, cmp_bt_sb;      // rows of a page are contiguous (512 elements apart)
    float sm_scale;
};

// What a token attends to, the same in every lane of its workgroup.
struct Token {
    int lo, nwin, limit, ncmp, total;         // first window key, window keys, causal limit of the compressed cache, slots / keys behind the window
    const int32_t *idx, *ori_bt, *cmp_bt;    // the token's index row (null: every compressed key below limit) and its sequence's table rows
    int64_t fallback;                        // byte address of the newest window key: where positions that do not count point
};

// The three steps from a list position to a row address.  kind: 0 = does not count, 1 = key of ori_kv, 2 = key of cmp_kv (a slot's value is
// judged in pick_block, one step after its load was issued).
struct Pick {
    int kind, key;
};
struct Block {
    int kind, blk, row;
};
struct Rows {
    int64_t addr;          // byte address of lane's row
    uint64_t counts;       // ballot of the positions that count
};

__device__ __forceinline__ Pick pick_key(const SskParams &p, const Token &tk, int tile, int t_end, int lane)
{
    const int pos = tile * kTile + lane;
    Pick r{0, 0};
    if (tile >= t_end || pos >= tk.total) return r;
    if (pos < tk.nwin) {
        r.kind = 1, r.key = tk.lo + pos;
    } else {
        r.kind = 2;
        r.key = tk.idx ? tk.idx[pos - tk.nwin] : pos - tk.nwin;
    }
    return r;
}
__device__ __forceinline__ Block pick_block(const SskParams &p, const Token &tk, const Pick &k)
{
    Block r{k.kind, 0, 0};
    if (k.kind == 2 && !(k.key >= 0 && k.key < tk.limit)) r.kind = 0;
    if (r.kind == 1) {
        const int page = k.key / p.ori_block;
        r.row = k.key - page * p.ori_block;
        r.blk = tk.ori_bt[page];
    } else if (r.kind == 2) {
        const int page = k.key / p.cmp_block;
        r.row = k.key - page * p.cmp_block;
        r.blk = tk.cmp_bt[page];
    }
    return r;
}
__device__ __forceinline__ Rows pick_rows(const SskParams &p, const Token &tk, const Block &k)
{
    Rows r;
    r.addr = tk.fallback;
    if (k.kind == 1) r.addr = (int64_t)(uintptr_t)p.ori_kv + 2 * ((int64_t)k.blk * p.ori_sblk + k.row * kDN);
    if (k.kind == 2) r.addr = (int64_t)(uintptr_t)p.cmp_kv + 2 * ((int64_t)k.blk * p.cmp_sblk + k.row * kDN);
    r.counts = __ballot(k.kind != 0);
    return r;
}
template <bool BF16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void sparse_sharedkv_kernel(SskParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int nsp = p.num_splits;
    const int64_t tok = blockIdx.x / nsp;
    const int split = blockIdx.x % nsp;
    const int head = wave * 16 + c16;

    // ---- the token's sequence, row and position
    int b, i, s1b;
    if (p.tnd) {
        int lo = 0, hi = p.batch;                                   // the sequence b with cu[b] <= tok < cu[b + 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)p.cu_q[mid + 1] <= tok) lo = mid + 1;
            else hi = mid;
        }
        b = lo;
        i = b < p.batch ? (int)(tok - p.cu_q[b]) : 0;
        s1b = b < p.batch ? p.cu_q[b + 1] - p.cu_q[b] : 0;
        if (b >= p.batch) b = 0, i = 0, s1b = 0;                    // behind the last sequence: a zero row
    } else {
        b = (int)(tok / p.s1), i = (int)(tok % p.s1);
        s1b = p.seqused_q ? min(max(p.seqused_q[b], 0), p.s1) : p.s1;
    }
    const int L = min(p.seqused_kv[b], p.ori_cap);
    const int pos_q = L - s1b + i;
    const int64_t q_off = p.tnd ? tok * p.q_ss : (int64_t)b * p.q_sb + (int64_t)i * p.q_ss;
    const int64_t o_off = p.tnd ? tok * p.o_ss : (int64_t)b * p.o_sb + (int64_t)i * p.o_ss;
    const int64_t slot = (tok * kHeads + head) * nsp + split;      // this head's partial
    const bool empty_row = i >= s1b || pos_q < 0 || L <= 0;

    Token tk;
    tk.lo = (int)max((int64_t)pos_q - p.win_left, (int64_t)0);
    tk.nwin = empty_row ? 0 : min((int)min((int64_t)pos_q + p.win_right, (int64_t)L - 1) - tk.lo + 1, p.ori_cap);
    tk.limit = p.cmp_kv ? min((pos_q + 1) / p.cmp_ratio, p.cmp_cap) : 0;
    tk.ncmp = !p.cmp_kv ? 0 : p.idx ? p.sparse_k : tk.limit;
    tk.total = empty_row ? 0 : tk.nwin + tk.ncmp;
    tk.idx = p.idx ? p.idx + (p.tnd ? tok * p.idx_ss : (int64_t)b * p.idx_sb + (int64_t)i * p.idx_ss) : nullptr;
    tk.ori_bt = p.ori_bt + (int64_t)b * p.ori_bt_sb;
    tk.cmp_bt = p.cmp_bt ? p.cmp_bt + (int64_t)b * p.cmp_bt_sb : nullptr;
    tk.fallback = 0;
    const int ntiles = (tk.total + kTile - 1) / kTile;
    const int tps = (ntiles + nsp - 1) / nsp;
    const int t_begin = min(split * tps, ntiles), t_end = min(t_begin + tps, ntiles);

    if (t_begin >= t_end) {      // a row that sees nothing, or a piece behind the token's last tile
        if (nsp == 1) {
            uint16_t *orow = p.out + o_off + (int64_t)head * p.o_sh + g * 128;
#pragma unroll
            for (int j = 0; j < 16; ++j) *(u32x4 *)(orow + j * 8) = u32x4{0u, 0u, 0u, 0u};
        } else if (g == 0) {
            // piece 0 of a row that sees keys always has a tile (the window holds the token's own key), so this is not the piece of the sink
            p.ws_ml[slot * 2 + 0] = -INFINITY;
            p.ws_ml[slot * 2 + 1] = 0.f;
        }
        return;
    }
    {      // the newest window key: a row the token may read, whatever else the tile holds
        const int n = tk.lo + tk.nwin - 1, page = n / p.ori_block;
        const int blk = tk.ori_bt[page];
        tk.fallback = (int64_t)(uintptr_t)p.ori_kv + 2 * ((int64_t)blk * p.ori_sblk + (n - page * p.ori_block) * kDN);
    }

    // Q^T fragments: lane (g, c16) holds q[head][ks*32 + g*8 .. +8]
    s16x8 qf[16];
    {
        const uint16_t *qrow = p.q + q_off + (int64_t)head * p.q_sh;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) qf[ks] = *(const s16x8 *)(qrow + ks * 32 + g * 8);
    }
    f32x4 acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // scaled log2 domain; the sink is a virtual key of logit sinks[h] (not multiplied by the scale) and value 0, owned by piece 0.  The
    // running reference starts a whole number and stays one (softmax_step<., true> has the reason).
    const float sink_l2 = p.sinks[head] * 1.4426950408889634f;
    float m_run = split == 0 ? ceilf(sink_l2) : -INFINITY;
    float l_run = split == 0 ? __builtin_amdgcn_exp2f(sink_l2 - m_run) : 0.f;

    // ---- prologue: tile t_begin into buffer 0; table entries of t_begin + 1 and indices of t_begin + 2 on their way
    Pick pk_a = pick_key(p, tk, t_begin, t_end, lane);
    Block bl_b = pick_block(p, tk, pk_a);
    pk_a = pick_key(p, tk, t_begin + 1, t_end, lane);
    Rows rows_cur = pick_rows(p, tk, bl_b);
    bl_b = pick_block(p, tk, pk_a);
    pk_a = pick_key(p, tk, t_begin + 2, t_end, lane);
    if (rows_cur.counts)
        for (int r = 0; r < 16; ++r) issue_nope_row(rows_cur.addr, wave + 4 * r, lds, lane);

    const float cs = p.sm_scale * 1.4426950408889634f;
    for (int t = t_begin; t < t_end; ++t) {
        uint8_t *buf = lds + ((t - t_begin) & 1) * kSskBuf;
        uint8_t *nbuf = lds + ((t + 1 - t_begin) & 1) * kSskBuf;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's rows of tile t have landed
        __syncthreads();                                      // tile t is complete in LDS, tile t-1 is no longer read
        const Rows rows_nxt = pick_rows(p, tk, bl_b);         // tile t + 1 (behind the piece: nothing counts, nothing is issued)
        // tile t + 2's table entries and tile t + 3's indices are asked for HERE, in front of the fill: what they return is first touched
        // behind the wait above of the next tile, so the compiler places no wait of its own between the fill and the MFMAs
        bl_b = pick_block(p, tk, pk_a);
        pk_a = pick_key(p, tk, t + 3, t_end, lane);
        const bool fill = rows_nxt.counts != 0;
        const uint64_t counts = rows_cur.counts;
        rows_cur = rows_nxt;
        // a tile that does not count computes nothing, so the fill of its successor is issued here at once.  (One fill site in front of the
        // branch, not inside the skipped arm: with the DMA statements in that arm the allocator spilled 138 registers per lane.)
        if (fill && counts == 0)
            for (int r = 0; r < 16; ++r) issue_nope_row(rows_nxt.addr, wave + 4 * r, nbuf, lane);
        if (counts == 0) continue;                            // nothing of this tile counts: it was not filled and is not computed

        // ---- S^T[key, head] = K . Q^T over 16 k-steps; tile t + 1 trickles in under the MFMAs
        f32x4 s[4];
        qk_scores<BF16, 16>([&](int ks, int mt) { return lda_nope(buf, ks, mt, g, c16); }, qf, s, [&](int ks) {
            if (fill) issue_nope_row(rows_nxt.addr, wave + 4 * ks, nbuf, lane);
        });
        // ---- lane owns keys mt*16 + 4g + r: the positions that do not count are masked
        if (~counts) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (!((counts >> (mt * 16 + 4 * g + r)) & 1ull)) s[mt][r] = -INFINITY;
        }
        s16x8 pf[2];
        softmax_step<BF16, true>(s, cs, m_run, l_run, acc, pf);
        pv_accumulate<BF16>(buf, pf, acc, g, c16);
    }

    if (nsp == 1) store_head_out<BF16>(p.out + o_off + (int64_t)head * p.o_sh, acc, l_run, g);
    else store_head_partial(p.ws_o + slot * kDN, p.ws_ml + slot * 2, acc, m_run, l_run, g);
}

// merge the partials of a token's pieces: one wave per (token, head), lane handles 8 of the 512 dims.  Piece 0 carries the sink in its
// (m, l); a piece that saw nothing carries (-inf, 0) and its O row is not read; a row whose pieces all saw nothing comes out as zeros.
template <bool BF16>
__global__ __launch_bounds__(256) void sparse_sharedkv_merge_kernel(SskParams p)
{
    const int lane = threadIdx.x & 63;
    const int64_t th = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (th >= p.tokens * kHeads) return;
    const int64_t tok = th / kHeads;
    const int h = (int)(th % kHeads), S = p.num_splits;
    int b = 0, i = 0;
    if (!p.tnd) b = (int)(tok / p.s1), i = (int)(tok % p.s1);
    const int64_t o_off = p.tnd ? tok * p.o_ss : (int64_t)b * p.o_sb + (int64_t)i * p.o_ss;
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, p.ws_ml[(th * S + s) * 2]);
    float Lsum = 0.f, o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
    for (int s = 0; s < S; ++s) {
        const float m = p.ws_ml[(th * S + s) * 2];
        if (m == -INFINITY) continue;
        const float w = __builtin_amdgcn_exp2f(m - M);
        Lsum += w * p.ws_ml[(th * S + s) * 2 + 1];
        const float *po = p.ws_o + (th * S + s) * kDN + lane * 8;
        const f32x4 a = *(const f32x4 *)po, c = *(const f32x4 *)(po + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] += w * a[j];
            o[4 + j] += w * c[j];
        }
    }
    const float inv = Lsum > 0.f ? 1.f / Lsum : 0.f;
    uint16_t *orow = p.out + o_off + (int64_t)h * p.o_sh + lane * 8;
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)cvt_out<BF16>(o[2 * j] * inv) | ((uint32_t)cvt_out<BF16>(o[2 * j + 1] * inv) << 16);
    *(u32x4 *)orow = w;
}

// pieces per token from host integers alone: at least one workgroup per CU, at least four tiles (256 list positions) per piece
int choose_splits(int64_t tokens, int64_t list_bound)
{
    if (tokens <= 0 || list_bound <= 0) return 1;
    const int64_t ntiles = (list_bound + kTile - 1) / kTile;
    const int cu = mi_gqa::cus();
    int64_t s = (cu + tokens - 1) / tokens;
    const int64_t cap = ntiles / 4 > 1 ? ntiles / 4 : 1;
    if (s > cap) s = cap;
    if (s > 32) s = 32;
    return s < 1 ? 1 : (int)s;
}

size_t partial_bytes(int64_t tokens, int num_splits)
{
    return num_splits <= 1 ? 0 : (size_t)tokens * kHeads * (size_t)num_splits * (kDN + 2) * sizeof(float);
}

}  // namespace
}  // namespace mi_sgl

using namespace mi_sgl;

extern "C" size_t mi_sparse_attn_sharedkv_workspace(int64_t tokens, int64_t list_bound, int num_splits)
{
    if (tokens <= 0 || list_bound <= 0 || num_splits < 0 || num_splits > kMaxSplits) return 0;
    return partial_bytes(tokens, num_splits ? num_splits : choose_splits(tokens, list_bound));
}

extern "C" int mi_sparse_attn_sharedkv(const void *q, const void *ori_kv, const void *cmp_kv, void *out, const float *sinks,
                                       const int32_t *cmp_sparse_indices, const int32_t *ori_block_table, const int32_t *cmp_block_table,
                                       const int32_t *cu_seqlens_q, const int32_t *seqused_q, const int32_t *seqused_kv, int layout_q,
                                       int batch, int s1, int64_t tokens, int heads, int head_dim, int ori_block, int ori_columns,
                                       int cmp_block, int cmp_columns, int sparse_count, int64_t q_stride_b, int64_t q_stride_s,
                                       int64_t q_stride_h, int64_t o_stride_b, int64_t o_stride_s, int64_t o_stride_h, int64_t idx_stride_b,
                                       int64_t idx_stride_s, int64_t ori_stride_blk, int64_t cmp_stride_blk, int64_t ori_bt_stride,
                                       int64_t cmp_bt_stride, float softmax_scale, int cmp_ratio, int ori_win_left, int ori_win_right,
                                       int dtype, int num_splits, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool tnd = layout_q == MI_SSK_Q_TND;
    if (layout_q != MI_SSK_Q_BSND && !tnd) return MI_SGL_EINVAL;
    if (heads != kHeads || head_dim != kDN) return MI_SGL_EINVAL;
    if (dtype != MI_DTYPE_BF16 && dtype != MI_DTYPE_F16) return MI_SGL_EINVAL;
    if (batch < 0 || tokens < 0 || (!tnd && (s1 < 0 || tokens != (int64_t)batch * s1))) return MI_SGL_EINVAL;
    if (ori_win_left < 0 || ori_win_right < 0 || !(softmax_scale >= 0.f) || !(softmax_scale < INFINITY)) return MI_SGL_EINVAL;
    auto block_ok = [](int blk) { return blk > 0 && blk <= 1024 && blk % 16 == 0; };
    if (!block_ok(ori_block) || ori_columns <= 0) return MI_SGL_EINVAL;
    if (cmp_sparse_indices && !cmp_kv) return MI_SGL_EINVAL;
    if (cmp_kv) {
        if (!cmp_block_table || !block_ok(cmp_block) || cmp_columns <= 0) return MI_SGL_EINVAL;
        if (cmp_ratio != 4 && cmp_ratio != 128) return MI_SGL_EINVAL;
        if (cmp_sparse_indices && (sparse_count < 1 || sparse_count > kMaxSparse)) return MI_SGL_EINVAL;
    }
    if (batch == 0 || tokens == 0) return MI_SGL_OK;
    if (!q || !ori_kv || !out || !sinks || !ori_block_table || !seqused_kv || (tnd && !cu_seqlens_q)) return MI_SGL_EINVAL;
    if (!mi_gqa::aligned8({q_stride_b, q_stride_s, q_stride_h, o_stride_b, o_stride_s, o_stride_h, ori_stride_blk, cmp_stride_blk}))
        return MI_SGL_EINVAL;      // 16-byte vector accesses
    const int64_t ori_cap = (int64_t)ori_columns * ori_block, cmp_cap = cmp_kv ? (int64_t)cmp_columns * cmp_block : 0;
    if (ori_cap > INT32_MAX || cmp_cap > INT32_MAX) return MI_SGL_EINVAL;
    const int64_t win = (int64_t)ori_win_left + ori_win_right + 1;
    const int64_t list_bound = (win < ori_cap ? win : ori_cap) + (cmp_sparse_indices ? sparse_count : cmp_cap);
    if (num_splits == 0) num_splits = choose_splits(tokens, list_bound);
    if (num_splits < 1 || num_splits > kMaxSplits || tokens * num_splits > INT32_MAX) return MI_SGL_EINVAL;
    if (num_splits > 1 && (!workspace || workspace_bytes < partial_bytes(tokens, num_splits))) return MI_SGL_EINVAL;

    SskParams p;
    p.q = (const uint16_t *)q, p.ori_kv = (const uint16_t *)ori_kv, p.cmp_kv = (const uint16_t *)cmp_kv, p.out = (uint16_t *)out;
    p.sinks = sinks, p.idx = cmp_sparse_indices, p.ori_bt = ori_block_table, p.cmp_bt = cmp_block_table;
    p.cu_q = cu_seqlens_q, p.seqused_q = tnd ? nullptr : seqused_q, p.seqused_kv = seqused_kv;
    p.ws_o = num_splits > 1 ? (float *)workspace : nullptr;
    p.ws_ml = num_splits > 1 ? p.ws_o + (size_t)tokens * kHeads * num_splits * kDN : nullptr;
    p.tnd = tnd, p.batch = batch, p.s1 = tnd ? 1 : s1, p.num_splits = num_splits, p.tokens = tokens;
    p.ori_block = ori_block, p.cmp_block = cmp_kv ? cmp_block : 1, p.ori_cap = (int)ori_cap, p.cmp_cap = (int)cmp_cap;
    p.sparse_k = cmp_sparse_indices ? sparse_count : 0, p.cmp_ratio = cmp_kv ? cmp_ratio : 1;
    p.win_left = ori_win_left, p.win_right = ori_win_right;
    p.q_sb = q_stride_b, p.q_ss = q_stride_s, p.q_sh = q_stride_h, p.o_sb = o_stride_b, p.o_ss = o_stride_s, p.o_sh = o_stride_h;
    p.idx_sb = idx_stride_b, p.idx_ss = idx_stride_s;
    p.ori_sblk = ori_stride_blk, p.cmp_sblk = cmp_stride_blk;
    p.ori_bt_sb = ori_bt_stride, p.cmp_bt_sb = cmp_bt_stride;
    p.sm_scale = softmax_scale;

    hipStream_t st = (hipStream_t)stream;
    constexpr size_t lds = 2 * (size_t)kSskBuf;
    static PerDeviceOnce attr_once;
    if (attr_once.need()) {
        (void)hipFuncSetAttribute((const void *)sparse_sharedkv_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void *)sparse_sharedkv_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    const dim3 grid((unsigned)(tokens * num_splits));
    if (dtype == MI_DTYPE_BF16) sparse_sharedkv_kernel<true><<<grid, 256, lds, st>>>(p);
    else sparse_sharedkv_kernel<false><<<grid, 256, lds, st>>>(p);
    if (num_splits > 1) {
        const dim3 mgrid((unsigned)((tokens * kHeads + 3) / 4));
        if (dtype == MI_DTYPE_BF16) sparse_sharedkv_merge_kernel<true><<<mgrid, 256, 0, st>>>(p);
        else sparse_sharedkv_merge_kernel<false><<<mgrid, 256, 0, st>>>(p);
    }
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}
