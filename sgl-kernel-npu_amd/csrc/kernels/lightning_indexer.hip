// hipcc-flags: -Rpass-analysis=kernel-resource-usage
// Lightning indexer of DeepSeek-V3.2 for gfx950: which KEYS (not blocks) should a query token attend to?  Replaces the reference's
// torch.ops.npu.lightning_indexer (csrc/lightning_indexer/: op_host/lightning_indexer.cpp, op_host/tiling/lightning_indexer_tiling.cpp,
// op_kernel/).  For a token with index-query Q [64, 128] and head weights w [64], and the keys K [S2, 128] of its sequence,
//
//     score[j] = sum_h w[h] * max(0, Q[h] . K[j])      (fp32)
//
// and the op returns the sparse_count best keys among those the token may see: descending score, ties by ascending key, -1 behind them.
//
// Two stream-ordered launches, both sized from host integers (shapes) only -- nothing is read back, the op replays in a captured graph:
//
//  score   a workgroup of 4 waves owns (group of TPW consecutive query rows, run of 64-key / 32-key stages); wave w takes the run's stages
//          w, w + 4, ...  Every wave keeps Q of the group's TPW tokens in registers (64 VGPRs a token) as the A operand of
//          mfma_f32_16x16x32 (S = Q.K^T, rows = heads) and loads 16 keys x 128 dims of a stage unit straight into the B operand (lane (g, c16):
//          key c16, dims ks*32 + 8g .. +8 -- every K byte is loaded once per workgroup, by one lane, and serves all TPW tokens).  Lane (g, c16)
//          then holds S[head 16 hb + 4g + r][key c16]: ReLU and the fp32 weights in-lane over r and the four head blocks hb, the four lane
//          rows meet in two permlane swaps.  Keys are masked by logical position against each row's own visible count (-inf); stages at or
//          behind the group's largest visible count are never looked up in the table and never loaded, rows of a loaded unit at or behind
//          it are zeros.  Loads run one stage ahead of the MFMAs in a second register set.  The rows of a TND group that belong to
//          different sequences are served one sequence after the other.  Scores go to an fp32 workspace [rows, ld].
//  select  a workgroup of 16 waves per row.  The 32-bit order-preserving image of a score (-0.0 counts as +0.0) is radix-selected, 8 bits a
//          pass over the row (which sits in L2), with one LDS histogram per wave; every wave owns a contiguous segment of the row, so the
//          last pass also leaves the number of threshold ties per segment.  One more pass compacts the keys above the threshold (any order)
//          and admits the ties in ascending key order until n = min(sparse_count, visible) is reached (ballot ranks inside a wave, segment
//          offsets across waves: an ordered scan, no atomic counter).  The n winners, as (descending image << 32 | key), are sorted in LDS
//          (bitonic, <= 2048 entries = 16 KB) and written, then -1.  visible <= sparse_count: every visible key wins, the radix is skipped.
//
// LIMITS (refused with MI_SGL_EINVAL, never a silent wrong answer): 64 heads, head dim 128, one key head; bf16 / fp16; 1 <= sparse_count
// <= 2048; sparse_mode 0 or 3; block_size a multiple of 16 up to 1024; s2_capacity <= MI_LIGHTNING_INDEXER_MAX_KEYS (262144).
#include <algorithm>
#include <stdlib.h>

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_score_dev.h"
#include "mi_sgl_kernels.h"

namespace mi_li {
using namespace mi_gqa;

constexpr int kHeads = 64, kDim = 128, kMaxSparse = 2048, kMaxKeys = MI_LIGHTNING_INDEXER_MAX_KEYS;
constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / 64;
constexpr size_t kDefaultWsBytes = (size_t)256 << 20;              // bound of the score workspace: larger inputs run in slices of rows

struct Params {
    const uint16_t *q, *k, *w;
    const int32_t *actq, *actk, *table;
    float *scores;                  // [rows of the slice, ld]
    int32_t *out;                   // [rows, sparse_count]
    int64_t q_s0, q_s1, q_sh, w_s0, w_s1, k_sblk, k_srow, tb_sr, ld;
    int q_tnd, k_layout, batch, inner;      // inner: S1 of a BSND query, 1 for TND
    int64_t rows;                   // B * S1 or T
    int cap, block_size, sparse_count, mode3;
    int64_t row_lo, group_lo;       // the slice: its first row (workspace row 0) and its first group
    int runs, stages_per_wg;
};

struct RowInfo {
    int b, visible, kbase;          // sequence; keys the row may see (0: none, nothing is computed); first key row of a TND key
};

// number of entries of the prefix sums cu[0 .. n) at or below t = the sequence token t belongs to; a whole wave calls it, the same in every lane
__device__ __forceinline__ int seq_of_token(const int32_t *cu, int n, int64_t t, int lane)
{
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        cnt += __popcll(__ballot(i < n && (int64_t)cu[min(i, n - 1)] <= t));
    }
    return cnt;
}

__device__ __forceinline__ RowInfo row_info(const Params &p, int64_t row, int lane)
{
    RowInfo ri{0, 0, 0};
    if (row >= p.rows) return ri;
    int b, r, s1;
    if (p.q_tnd) {
        b = seq_of_token(p.actq, p.batch, row, lane);
        if (b >= p.batch) return ri;                              // a token behind the last prefix sum belongs to no sequence
        const int start = b ? p.actq[b - 1] : 0;
        s1 = p.actq[b] - start, r = (int)(row - start);
    } else {
        b = (int)(row / p.inner), r = (int)(row % p.inner);
        s1 = p.actq ? min(max(p.actq[b], 0), p.inner) : p.inner;
        if (r >= s1) return ri;
    }
    ri.b = b;
    int s2 = p.cap;
    if (p.k_layout == MI_LI_KEY_TND) {
        ri.kbase = b ? p.actk[b - 1] : 0;
        s2 = min(p.actk[b] - ri.kbase, p.cap - ri.kbase);
        if (ri.kbase < 0) s2 = 0;
    } else if (p.actk) {
        s2 = p.actk[b];
    }
    s2 = min(max(s2, 0), p.cap);
    ri.visible = p.mode3 ? min(max(s2 - (s1 - 1 - r), 0), s2) : s2;
    return ri;
}

__device__ __forceinline__ int64_t row_offset(int64_t row, int inner, int64_t s0, int64_t s1) { return (row / inner) * s0 + (row % inner) * s1; }

template <bool BF16>
__device__ __forceinline__ float to_f32(uint16_t v)
{
    if constexpr (BF16) return __uint_as_float((uint32_t)v << 16);
    else return (float)__builtin_bit_cast(_Float16, v);
}

// TPW: query rows of a group (their Q fragments live in every wave); UP: 16-key units of a load stage
template <bool BF16, int TPW, int UP>
__global__ __launch_bounds__(256) void lightning_score_kernel(Params p)
{
    constexpr int HB = kHeads / 16, QS = kDim / 32, SK = UP * 16;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int run = blockIdx.x % p.runs;
    const int64_t grp = p.group_lo + blockIdx.x / p.runs;

    // the group's rows
    int64_t row[TPW];
    int bs_[TPW], vis[TPW], kb[TPW];
    unsigned remaining = 0;
    int vis_all = 0;
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        if (p.q_tnd) {
            row[s] = grp * TPW + s;
        } else {
            const int gps = (p.inner + TPW - 1) / TPW;
            const int sq = (int)(grp % gps) * TPW + s;
            row[s] = sq < p.inner ? (grp / gps) * p.inner + sq : p.rows;
        }
        const RowInfo ri = row_info(p, row[s], lane);
        bs_[s] = __builtin_amdgcn_readfirstlane(ri.b), vis[s] = __builtin_amdgcn_readfirstlane(ri.visible);
        kb[s] = __builtin_amdgcn_readfirstlane(ri.kbase);
        if (vis[s] > 0) remaining |= 1u << s;
        vis_all = max(vis_all, vis[s]);
    }
    const int st_first = run * p.stages_per_wg + wave;            // this wave's stages: st_first, st_first + 4, ... below the run's end
    if ((int64_t)st_first * SK >= vis_all) return;                // no LDS, no barrier: waves are on their own

    // Q fragments (A operand): lane (g, c16) holds q[head 16 hb + c16][ks*32 + 8g .. +8]; weights of the heads 16 hb + 4g + r it sums
    s16x8 qf[TPW][HB][QS];
    float wf[TPW][HB][4];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        const bool ok = (remaining >> s) & 1;
        const int64_t rr = ok ? row[s] : 0;
        const uint16_t *qrow = p.q + row_offset(rr, p.inner, p.q_s0, p.q_s1);
        const uint16_t *wrow = p.w + row_offset(rr, p.inner, p.w_s0, p.w_s1);
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
#pragma unroll
            for (int ks = 0; ks < QS; ++ks)
                qf[s][hb][ks] = ok ? *(const s16x8 *)(qrow + (int64_t)(hb * 16 + c16) * p.q_sh + ks * 32 + g * 8) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
            const uint2 wv = ok ? *(const uint2 *)(wrow + hb * 16 + 4 * g) : uint2{0u, 0u};
            wf[s][hb][0] = to_f32<BF16>((uint16_t)(wv.x & 0xffff)), wf[s][hb][1] = to_f32<BF16>((uint16_t)(wv.x >> 16));
            wf[s][hb][2] = to_f32<BF16>((uint16_t)(wv.y & 0xffff)), wf[s][hb][3] = to_f32<BF16>((uint16_t)(wv.y >> 16));
        }
    }

    while (remaining) {                                           // one turn per sequence of the group (BSND: one)
        int b = 0, kbase = 0, vmax = 0;
        unsigned act = 0;
        bool first = true;
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
            if (!((remaining >> s) & 1)) continue;
            if (first) b = bs_[s], kbase = kb[s], first = false;
            if (bs_[s] == b) act |= 1u << s, vmax = max(vmax, vis[s]);
        }
        remaining &= ~act;
        const int st_end = min((run + 1) * p.stages_per_wg, (vmax + SK - 1) / SK);
        if (st_first >= st_end) continue;

        // stage st: keys st*SK .. +SK; unit i: keys st*SK + 16 i .. +16, lane loads dims ks*32 + 8g .. +8 of key c16.  The pages of a stage's
        // units are looked up by its first lanes and read lane by lane.
        auto load_stage = [&](int st, u32x4(&kr)[UP][QS]) {
            const int pos_l = st * SK + (lane & (UP - 1)) * 16;
            int64_t base_l = 0;                                   // element offset of the unit's first key row
            if (st < st_end && pos_l < vmax) {
                if (p.k_layout == MI_LI_KEY_PA_BSND) {
                    const unsigned blk = (unsigned)pos_l / (unsigned)p.block_size;
                    const int64_t page = p.table[(int64_t)b * p.tb_sr + blk];
                    base_l = page * p.k_sblk + (int64_t)(pos_l - (int)blk * p.block_size) * p.k_srow;
                } else {
                    base_l = (p.k_layout == MI_LI_KEY_BSND ? (int64_t)b * p.k_sblk : 0) + ((int64_t)kbase + pos_l) * p.k_srow;
                }
            }
            const int base_lo = (int)(uint32_t)base_l, base_hi = (int)(base_l >> 32);
#pragma unroll
            for (int i = 0; i < UP; ++i) {
                const int64_t base = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(base_hi, i) << 32) |
                                               (uint32_t)__builtin_amdgcn_readlane(base_lo, i));
                const bool ok = st < st_end && st * SK + i * 16 + c16 < vmax;      // rows behind the largest visible count are zeros, never read
                const uint16_t *krow = p.k + base + (int64_t)c16 * p.k_srow;
#pragma unroll
                for (int ks = 0; ks < QS; ++ks) kr[i][ks] = ok ? *(const u32x4 *)(krow + ks * 32 + g * 8) : u32x4{0, 0, 0, 0};
            }
        };

        auto compute_stage = [&](int st, const u32x4(&kr)[UP][QS]) {
            if (st >= st_end) return;                             // wave-uniform
#pragma unroll
            for (int s = 0; s < TPW; ++s) {
                if (!((act >> s) & 1)) continue;                  // wave-uniform
                float mine = -INFINITY;                           // lane (g, c16), g < UP, stores key st*SK + 16 g + c16
#pragma unroll
                for (int i = 0; i < UP; ++i) {
                    f32x4 acc[HB];
#pragma unroll
                    for (int hb = 0; hb < HB; ++hb) {
                        acc[hb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ks = 0; ks < QS; ++ks) acc[hb] = mfma16<BF16>(qf[s][hb][ks], __builtin_bit_cast(s16x8, kr[i][ks]), acc[hb]);
                    }
                    float tot = 0.f;
#pragma unroll
                    for (int hb = 0; hb < HB; ++hb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) tot += wf[s][hb][r] * fmaxf(acc[hb][r], 0.f);
                    tot = sum_over_rows(tot);                     // every lane of column c16 holds the key's score
                    if (g == i) mine = st * SK + i * 16 + c16 < vis[s] ? tot : -INFINITY;
                }
                if (g < UP) p.scores[(row[s] - p.row_lo) * p.ld + st * SK + g * 16 + c16] = mine;
            }
        };

        u32x4 ka[UP][QS], kc[UP][QS];
        load_stage(st_first, ka);
        for (int st = st_first; st < st_end; st += 8) {
            load_stage(st + 4, kc);                               // travels under the MFMAs of the stage before it
            compute_stage(st, ka);
            load_stage(st + 8, ka);
            compute_stage(st + 4, kc);
        }
    }
}

__device__ __forceinline__ uint32_t score_image(float s)          // ascending: a larger score has a larger image; -0.0 == +0.0
{
    uint32_t u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

// one workgroup of 16 waves per row of the slice
__global__ __launch_bounds__(kSelThreads) void lightning_select_kernel(Params p)
{
    __shared__ uint64_t cand[kMaxSparse];
    __shared__ int hist[kSelWaves][256];
    __shared__ int bins[256];
    __shared__ int ctl[4];                                        // [0] digit found, [1] remaining rank, [2] cursor of the keys above
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row = p.row_lo + blockIdx.x;
    const RowInfo ri = row_info(p, row, lane);
    const int visible = __builtin_amdgcn_readfirstlane(ri.visible);
    const int K = p.sparse_count, n = min(K, visible);
    int32_t *orow = p.out + row * K;
    if (n == 0) {
        for (int t = tid; t < K; t += kSelThreads) orow[t] = -1;
        return;
    }
    const float *srow = p.scores + (row - p.row_lo) * p.ld;
    // wave w owns keys [seg0, seg1): a multiple of 64 each, so that a wave reads whole 256-byte lines
    const int seg = ((visible + kSelWaves - 1) / kSelWaves + 63) / 64 * 64;
    const int seg0 = min(wave * seg, visible), seg1 = min(seg0 + seg, visible);

    uint32_t thr = 0;                                             // image of the n-th largest score
    int need = n;                                                 // ties at the threshold to admit; visible <= K: everything wins
    bool all = visible <= K;
    if (!all) {
        uint32_t prefix = 0, pmask = 0;
        int rank = n;                                             // the rank-th largest among the keys that match the prefix
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int t = tid; t < kSelWaves * 256; t += kSelThreads) (&hist[0][0])[t] = 0;
            __syncthreads();
            for (int j = seg0 + lane; j < seg1; j += 64) {
                const uint32_t u = score_image(srow[j]);
                if ((u & pmask) == prefix) atomicAdd(&hist[wave][(u >> shift) & 255], 1);
            }
            __syncthreads();
            if (tid < 256) {
                int c = 0;
#pragma unroll
                for (int w = 0; w < kSelWaves; ++w) c += hist[w][tid];
                bins[tid] = c;
            }
            __syncthreads();
            if (tid < 256) {                                      // keys with a larger digit than mine
                int above = 0;
                for (int d = tid + 1; d < 256; ++d) above += bins[d];
                if (above < rank && rank <= above + bins[tid]) ctl[0] = tid, ctl[1] = rank - above;
            }
            __syncthreads();
            const int d = ctl[0] & 255;
            rank = ctl[1];
            prefix |= (uint32_t)d << shift, pmask |= 255u << shift;
            if (shift == 0) {                                     // hist[w][d]: the threshold ties of wave w's segment
                thr = prefix, need = rank;
            }
        }
    }
    if (tid == 0) ctl[2] = 0;
    // ties of the segments before mine (the last pass's histograms are still in place)
    int tie_base = 0;
    if (!all) {
        const int d = thr & 255;
        for (int w = 0; w < wave; ++w) tie_base += hist[w][d];
    }
    const int n_above = n - need;                                 // keys strictly above the threshold (all: unused)
    __syncthreads();
    for (int j0 = seg0; j0 < seg1; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < seg1;
        const uint32_t u = in ? score_image(srow[j]) : 0u;
        const uint64_t key = ((uint64_t)(~u) << 32) | (uint32_t)j;    // smaller = better: higher score first, then the lower key
        if (all) {
            if (in) cand[j] = key;
        } else {
            if (in && u > thr) {
                const int at = atomicAdd(&ctl[2], 1);            // exactly n_above keys lie above the threshold
                if (at < n_above) cand[at] = key;
            }
            const uint64_t ties = __ballot(in && u == thr);
            if (in && u == thr) {
                const int rk = tie_base + __popcll(ties & ((1ull << lane) - 1));
                if (rk < need) cand[n_above + rk] = key;
            }
            tie_base += __popcll(ties);
        }
    }
    int P = 2;
    while (P < n) P *= 2;
    for (int t = n + tid; t < P; t += kSelThreads) cand[t] = ~0ull;
    __syncthreads();
    bitonic_sort<kSelThreads>(cand, P);
    for (int t = tid; t < K; t += kSelThreads) orow[t] = t < n ? (int32_t)(uint32_t)cand[t] : -1;
}

static size_t ws_bound()                                          // MI_LIGHTNING_INDEXER_WS_BYTES lowers (or raises) the bound: tests use it
{
    const char *e = getenv("MI_LIGHTNING_INDEXER_WS_BYTES");
    if (e && *e) {
        const long long v = atoll(e);
        if (v > 0) return (size_t)v;
    }
    return kDefaultWsBytes;
}

static int64_t score_ld(int64_t cap) { return (cap + 63) / 64 * 64; }

// rows per group: one when no sequence can hold two query rows (decode), otherwise four that share every K load
static int tokens_per_group(int layout_query, int batch, int s1, int64_t rows)
{
    if (layout_query == MI_LI_QUERY_BSND) return s1 > 1 ? 4 : 1;
    return rows > batch ? 4 : 1;
}
static int64_t group_count(int layout_query, int batch, int s1, int64_t rows, int tpw)
{
    return layout_query == MI_LI_QUERY_BSND ? (int64_t)batch * ((s1 + tpw - 1) / tpw) : (rows + tpw - 1) / tpw;
}
static int64_t group_first_row(int layout_query, int s1, int64_t grp, int tpw)
{
    if (layout_query != MI_LI_QUERY_BSND) return grp * tpw;
    const int gps = (s1 + tpw - 1) / tpw;
    return (grp / gps) * s1 + (grp % gps) * tpw;
}
// groups a slice of the workspace bound holds (at least one): a group spans at most tpw rows of ld floats
static int64_t groups_per_slice(int64_t ld, int tpw, size_t bound) { return std::max<int64_t>(1, (int64_t)(bound / ((size_t)ld * 4 * tpw))); }

struct Args {
    const void *q, *k, *w;
    const int32_t *actq, *actk, *table;
    int layout_query, layout_key, batch, s1;
    int64_t rows;
    int heads, key_heads, head_dim;
    int64_t cap;
    int block_size;
    int64_t tb_sr, q_s0, q_s1, q_sh, w_s0, w_s1, k_sblk, k_srow;
    int sparse_count, sparse_mode, dtype;
};

static int check(const Args &a)
{
    if (a.layout_query != MI_LI_QUERY_BSND && a.layout_query != MI_LI_QUERY_TND) return MI_SGL_EINVAL;
    if (a.layout_key != MI_LI_KEY_BSND && a.layout_key != MI_LI_KEY_TND && a.layout_key != MI_LI_KEY_PA_BSND) return MI_SGL_EINVAL;
    if (a.layout_key != MI_LI_KEY_PA_BSND && a.layout_key != a.layout_query) return MI_SGL_EINVAL;      // non-paged: the layouts are equal
    if (a.key_heads != 1 || a.heads != kHeads * a.key_heads || a.head_dim != kDim) return MI_SGL_EINVAL;
    if (a.dtype != MI_DTYPE_BF16 && a.dtype != MI_DTYPE_F16) return MI_SGL_EINVAL;
    if (a.sparse_count < 1 || a.sparse_count > kMaxSparse) return MI_SGL_EINVAL;
    if (a.sparse_mode != 0 && a.sparse_mode != 3) return MI_SGL_EINVAL;
    if (a.batch < 0 || a.rows < 0 || a.cap < 1 || a.cap > kMaxKeys) return MI_SGL_EINVAL;                 // the declared limit
    if (a.layout_query == MI_LI_QUERY_BSND && (a.s1 < 1 || a.rows != (int64_t)a.batch * a.s1)) return MI_SGL_EINVAL;
    if (a.layout_query == MI_LI_QUERY_TND && !a.actq && a.rows > 0) return MI_SGL_EINVAL;
    if (a.layout_key == MI_LI_KEY_PA_BSND) {
        if (a.block_size < 16 || a.block_size > 1024 || a.block_size % 16) return MI_SGL_EINVAL;
        if ((!a.table || !a.actk) && a.rows > 0) return MI_SGL_EINVAL;
        if (a.cap % a.block_size) return MI_SGL_EINVAL;           // table columns * block_size
    } else if (a.table) {
        return MI_SGL_EINVAL;
    }
    if (a.layout_key == MI_LI_KEY_TND && !a.actk && a.rows > 0) return MI_SGL_EINVAL;
    if (a.rows == 0 || a.batch == 0) return MI_SGL_OK;
    if (!a.q || !a.k || !a.w) return MI_SGL_EINVAL;
    if ((a.q_s0 % 8) || (a.q_s1 % 8) || (a.q_sh % 8) || (a.k_sblk % 8) || (a.k_srow % 8) || (a.w_s0 % 4) || (a.w_s1 % 4)) return MI_SGL_EINVAL;
    if (((uintptr_t)a.q & 15) || ((uintptr_t)a.k & 15) || ((uintptr_t)a.w & 7)) return MI_SGL_EINVAL;    // 16-byte / 8-byte loads
    return MI_SGL_OK;
}

static Params make_params(const Args &a)
{
    Params p;
    p.q = (const uint16_t *)a.q, p.k = (const uint16_t *)a.k, p.w = (const uint16_t *)a.w;
    p.actq = a.actq, p.actk = a.actk, p.table = a.table;
    p.scores = nullptr, p.out = nullptr;
    p.q_s0 = a.q_s0, p.q_s1 = a.q_s1, p.q_sh = a.q_sh, p.w_s0 = a.w_s0, p.w_s1 = a.w_s1, p.k_sblk = a.k_sblk, p.k_srow = a.k_srow;
    p.tb_sr = a.tb_sr, p.ld = score_ld(a.cap);
    p.q_tnd = a.layout_query == MI_LI_QUERY_TND, p.k_layout = a.layout_key, p.batch = a.batch, p.inner = p.q_tnd ? 1 : a.s1;
    p.rows = a.rows, p.cap = (int)a.cap, p.block_size = a.block_size, p.sparse_count = a.sparse_count, p.mode3 = a.sparse_mode == 3;
    p.row_lo = 0, p.group_lo = 0, p.runs = 1, p.stages_per_wg = 4;
    return p;
}

template <bool BF16>
static void launch_score_dtype(const Params &p, int tpw, unsigned grid, hipStream_t st)
{
    if (tpw == 1) lightning_score_kernel<BF16, 1, 4><<<grid, 256, 0, st>>>(p);
    else lightning_score_kernel<BF16, 4, 2><<<grid, 256, 0, st>>>(p);
}

// the score launch over groups [g0, g1): about eight workgroups per CU, a wave with at least one stage
static int launch_score(Params p, const Args &a, int tpw, int64_t g0, int64_t g1, hipStream_t st)
{
    const int sk = tpw == 1 ? 64 : 32;
    const int64_t stages = (a.cap + sk - 1) / sk, chunks = (stages + 3) / 4, cells = g1 - g0;
    int64_t runs = std::min<int64_t>((8ll * cus() + cells - 1) / cells, chunks);
    runs = std::max<int64_t>(runs, 1);
    p.stages_per_wg = (int)((chunks + runs - 1) / runs * 4);
    p.runs = (int)((stages + p.stages_per_wg - 1) / p.stages_per_wg);
    p.group_lo = g0, p.row_lo = group_first_row(a.layout_query, a.s1, g0, tpw);
    const int64_t wgs = cells * p.runs;
    if (wgs > 0x7fffffffll) return MI_SGL_EINVAL;
    if (a.dtype == MI_DTYPE_BF16) launch_score_dtype<true>(p, tpw, (unsigned)wgs, st);
    else launch_score_dtype<false>(p, tpw, (unsigned)wgs, st);
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}

}  // namespace mi_li

using namespace mi_li;

extern "C" size_t mi_lightning_indexer_workspace(int layout_query, int batch, int s1, int64_t rows, int64_t s2_capacity)
{
    if (batch <= 0 || rows <= 0 || s2_capacity <= 0 || s2_capacity > kMaxKeys) return 0;
    if (layout_query == MI_LI_QUERY_BSND && s1 < 1) return 0;
    const int tpw = tokens_per_group(layout_query, batch, s1, rows);
    const int64_t ld = score_ld(s2_capacity);
    const int64_t groups = std::min(group_count(layout_query, batch, s1, rows, tpw), groups_per_slice(ld, tpw, ws_bound()));
    return (size_t)groups * tpw * ld * sizeof(float);
}

extern "C" int mi_lightning_indexer_score(const void *query, const void *key, const void *weights, float *scores, int64_t score_stride,
                                          const int32_t *actual_seq_lengths_query, const int32_t *actual_seq_lengths_key,
                                          const int32_t *block_table, int layout_query, int layout_key, int batch, int s1, int64_t rows,
                                          int heads, int key_heads, int head_dim, int64_t s2_capacity, int block_size, int64_t bt_stride_b,
                                          int64_t q_stride_0, int64_t q_stride_1, int64_t q_stride_h, int64_t w_stride_0, int64_t w_stride_1,
                                          int64_t k_stride_blk, int64_t k_stride_row, int sparse_mode, int dtype, void *stream)
{
    const Args a{query, key, weights, actual_seq_lengths_query, actual_seq_lengths_key, block_table, layout_query, layout_key, batch, s1, rows,
                 heads, key_heads, head_dim, s2_capacity, block_size, bt_stride_b, q_stride_0, q_stride_1, q_stride_h, w_stride_0, w_stride_1,
                 k_stride_blk, k_stride_row, 1, sparse_mode, dtype};
    const int rc = check(a);
    if (rc != MI_SGL_OK || rows == 0 || batch == 0) return rc;
    if (!scores || ((uintptr_t)scores & 3) || score_stride < score_ld(s2_capacity)) return MI_SGL_EINVAL;
    Params p = make_params(a);
    p.scores = scores, p.ld = score_stride;
    const int tpw = tokens_per_group(layout_query, batch, s1, rows);
    return launch_score(p, a, tpw, 0, group_count(layout_query, batch, s1, rows, tpw), (hipStream_t)stream);
}

extern "C" int mi_lightning_indexer(const void *query, const void *key, const void *weights, int32_t *sparse_indices,
                                    const int32_t *actual_seq_lengths_query, const int32_t *actual_seq_lengths_key, const int32_t *block_table,
                                    int layout_query, int layout_key, int batch, int s1, int64_t rows, int heads, int key_heads, int head_dim,
                                    int64_t s2_capacity, int block_size, int64_t bt_stride_b, int64_t q_stride_0, int64_t q_stride_1,
                                    int64_t q_stride_h, int64_t w_stride_0, int64_t w_stride_1, int64_t k_stride_blk, int64_t k_stride_row,
                                    int sparse_count, int sparse_mode, int dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    const Args a{query, key, weights, actual_seq_lengths_query, actual_seq_lengths_key, block_table, layout_query, layout_key, batch, s1, rows,
                 heads, key_heads, head_dim, s2_capacity, block_size, bt_stride_b, q_stride_0, q_stride_1, q_stride_h, w_stride_0, w_stride_1,
                 k_stride_blk, k_stride_row, sparse_count, sparse_mode, dtype};
    const int rc = check(a);
    if (rc != MI_SGL_OK || rows == 0 || batch == 0) return rc;
    if (!sparse_indices) return MI_SGL_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 3) ||
        workspace_bytes < mi_lightning_indexer_workspace(layout_query, batch, s1, rows, s2_capacity))
        return MI_SGL_EINVAL;
    Params p = make_params(a);
    p.scores = (float *)workspace, p.out = sparse_indices;
    const int tpw = tokens_per_group(layout_query, batch, s1, rows);
    const int64_t groups = group_count(layout_query, batch, s1, rows, tpw), per = groups_per_slice(p.ld, tpw, ws_bound());
    hipStream_t st = (hipStream_t)stream;
    for (int64_t g0 = 0; g0 < groups; g0 += per) {                // slices of rows: the workspace is reused, the stream orders them
        const int64_t g1 = std::min(groups, g0 + per);
        const int rs = launch_score(p, a, tpw, g0, g1, st);
        if (rs != MI_SGL_OK) return rs;
        p.row_lo = group_first_row(layout_query, s1, g0, tpw);
        const int64_t row_hi = g1 == groups ? rows : group_first_row(layout_query, s1, g1, tpw);
        if (row_hi - p.row_lo > 0x7fffffffll) return MI_SGL_EINVAL;
        lightning_select_kernel<<<(unsigned)(row_hi - p.row_lo), kSelThreads, 0, st>>>(p);
        if (hipGetLastError() != hipSuccess) return MI_SGL_ELAUNCH;
    }
    return MI_SGL_OK;
}
