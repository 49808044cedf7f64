// compressor for gfx950 (MI355X), bf16 / fp16: the producer of DeepSeek's compressed-KV cache that lightning_indexer.hip selects from and
// sparse_sharedkv.hip attends over.  Replaces the reference's AscendC op csrc/compressor/ (op_kernel/compressor_block_{cube,vec}_perf.h); the
// semantics are stated in include/mi_sgl_kernels.h and DESIGN.md 4.3.7.
//
// Four launches on one stream, nothing read back by the host (grids come from T, B and the output row count):
//  * plan      one workgroup: the number of groups each sequence completes in this call and its exclusive prefix sum -- where a sequence's
//              rows start in the packed TH output -- into the head of the workspace;
//  * project   P[T, 2 ww] = x[T, H] . [wkv; wgate]^T in fp32 on 16x16x32 MFMAs.  Both operands are K-contiguous, so the A and the B fragment
//              are the same 16-byte read; wkv and wgate stay two tensors, a column tile picks its base pointer.  Tiles of (BM + BN) rows x 64
//              k go global -> LDS by LDS-DMA at 16 bytes, 8 rows of 128 B per wave-instruction, one barrier per tile, two buffers in the
//              large form and four in the skinny one (three tiles in flight across the barriers, waited for by count); the
//              16-byte chunks of a row are XOR-swizzled on the SOURCE address (the LDS image of a DMA is lane-linear) and the reads undo it.
//              Two forms: 128 x 128 (4 waves as 2 x 2, 4 x 4 accumulators each) for T > 256, 128 x 32 (4 waves down M) for T <= 256, where
//              the weights bound the time and 2 ww / 32 column tiles times a K split fill the chip.  A K split writes one fp32 slab per
//              piece; the consumers add the slabs in slab order (no float atomics: the same bits from run to run);
//  * compress  one workgroup per output slot, lane = channel: online softmax over the coff * r stacked rows in fp32 (a row comes from the
//              slabs where its position is at or behind start_pos, from state_cache where it is before, and is (0, -inf) before position
//              0), RMSNorm through one block reduction, RoPE on the last 64 channels through LDS, cast, store.  An empty slot stores zeros;
//  * save      one workgroup per token row: [kv | score + ape] into state_cache under the rules of the cache mode.
// save is enqueued BEHIND compress: a history row is read before this call can overwrite it (ring tables map position p and p + capacity to
// one slot).  What remains is the reference's precondition: the table maps no two positions this call writes to one slot.
#include "device_once.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mi_sgl_kernels.h"
#include "gqa_common.h"      // cus()
#include "latent_tile_dev.h" // dma_row, mfma16, cvt_out

namespace mi_sgl {
namespace {

constexpr int kBK = 64;                  // k elements per tile: 128 B per row, 8 chunks of 16 B
constexpr int kRowBytes = kBK * 2;
constexpr int kSkinnyRows = 256;         // T at or below: the 128 x 32 form
constexpr int kMaxKSplit = 8;
constexpr int kPlanThreads = 256;

struct CmpParams {
    const uint16_t *x, *wkv, *wgate;
    float *state;
    const float *ape, *norm_w, *rope_sin, *rope_cos;
    const int32_t *table, *cu, *seqused, *start_pos;
    uint16_t *out;
    int32_t *group_off;      // [batch + 1] exclusive prefix of the groups a sequence completes (workspace head)
    float *slabs;            // [ksplit][T][2 ww] fp32
    int64_t tokens, out_rows, state_rows;      // state_rows = blocks * block_size
    int batch, seq, th, hidden, d, ww, r, coff, rotary, cache_mode, block_size, table_cols, ksplit, cg;
    int64_t state_blocks, table_stride;
    float eps;
};

// ---- what a sequence contributes: span, used tokens, start, first token row
struct Seq {
    int base, used, start;
};
__device__ __forceinline__ Seq seq_of(const CmpParams &p, int b)
{
    Seq s;
    const int span = p.th ? p.cu[b + 1] - p.cu[b] : p.seq;
    s.base = p.th ? p.cu[b] : b * p.seq;
    s.used = p.seqused ? min(max(p.seqused[b], 0), max(span, 0)) : max(span, 0);
    s.start = p.start_pos ? max(p.start_pos[b], 0) : 0;
    return s;
}
__device__ __forceinline__ int groups_of(const CmpParams &p, const Seq &s)
{
    return (int)(((int64_t)s.start + s.used) / p.r) - s.start / p.r;
}

__global__ __launch_bounds__(kPlanThreads) void compressor_plan_kernel(CmpParams p)
{
    __shared__ int part[kPlanThreads];
    const int t = threadIdx.x, per = (p.batch + kPlanThreads - 1) / kPlanThreads;
    const int lo = min(t * per, p.batch), hi = min(lo + per, p.batch);
    int sum = 0;
    for (int b = lo; b < hi; ++b) sum += groups_of(p, seq_of(p, b));
    part[t] = sum;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < t; ++i) off += part[i];
    for (int b = lo; b < hi; ++b) {
        p.group_off[b] = off;
        off += groups_of(p, seq_of(p, b));
    }
    if (t == kPlanThreads - 1) p.group_off[p.batch] = off;
}

// ---- projection GEMM
template <bool BF16, int WM, int WN, int MT, int NT, int NBUF>
__global__ __launch_bounds__(256) void compressor_gemm_kernel(CmpParams p)
{
    constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
    constexpr int kBuf = (BM + BN) * kRowBytes;
    constexpr int NI = (BM + BN) / 8 / 4;      // DMA instructions per wave and tile (8 rows each)
    static_assert(WM * WN == 4 && (BM + BN) % 32 == 0, "four waves");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int wm = wave / WN, wn = wave % WN;
    const int n2 = 2 * p.ww, ntiles = n2 / BN;
    const int n_tile = blockIdx.x % ntiles, rest = blockIdx.x / ntiles;
    const int split = rest % p.ksplit, m_tile = rest / p.ksplit;
    const int64_t m0 = (int64_t)m_tile * BM;
    const int n0 = n_tile * BN;
    const int kper = p.hidden / p.ksplit, nk = kper / kBK;
    const uint16_t *wb = n0 < p.ww ? p.wkv + (int64_t)n0 * p.hidden : p.wgate + (int64_t)(n0 - p.ww) * p.hidden;

    // lane's source of DMA instruction wave + 4 j: row 8 (wave + 4 j) + (lane >> 3) of the tile, the 16-byte chunk that belongs in slot lane & 7
    const uint8_t *src[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int row = (wave + 4 * j) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ (row & 7);
        const uint16_t *base;
        if (row < BM) {
            const int64_t gr = min(m0 + row, p.tokens - 1);      // rows behind T: a valid address, the result is not stored
            base = p.x + gr * p.hidden;
        } else {
            base = wb + (int64_t)(row - BM) * p.hidden;
        }
        src[j] = (const uint8_t *)(base + (int64_t)split * kper) + chunk * 16;
    }
    auto fill = [&](uint8_t *buf) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            dma_row(buf + (wave + 4 * j) * 1024, src[j]);
            src[j] += kRowBytes;
        }
    };
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // NBUF - 1 tiles are in flight ahead of the one computed on.  Tile kt is waited for by COUNT (the DMAs of the tiles behind it stay in
    // flight across the barrier; in the last NBUF - 2 iterations fewer are behind it and the wait is for all), and the barrier is the raw
    // one: __syncthreads() would drain the queue.  Tile kt + NBUF - 1 goes into the buffer tile kt - 1 was read from, behind that barrier.
    const int pre = nk < NBUF - 1 ? nk : NBUF - 1;
    for (int t = 0; t < pre; ++t) fill(lds + t * kBuf);
    for (int kt = 0; kt < nk; ++kt) {
        const uint8_t *buf = lds + (kt % NBUF) * kBuf;
        if (kt + NBUF - 1 <= nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * NI) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // tile kt is whole, tile kt - 1 is no longer read
        if (kt + NBUF - 1 < nk) fill(lds + ((kt + NBUF - 1) % NBUF) * kBuf);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            s16x8 a[MT], b[NT];
            const int slot = ((ks * 4 + g) ^ (c16 & 7)) * 16;      // every fragment row is c16 mod 8
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = *(const s16x8 *)(buf + ((wm * MT + i) * 16 + c16) * kRowBytes + slot);
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = *(const s16x8 *)(buf + (BM + (wn * NT + j) * 16 + c16) * kRowBytes + slot);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = mfma16<BF16>(a[i], b[j], acc[i][j]);
        }
    }
    // lane holds C[m0 + (wm MT + i) 16 + 4 g + r][n0 + (wn NT + j) 16 + c16]
    float *slab = p.slabs + (int64_t)split * p.tokens * n2;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + (wm * MT + i) * 16 + 4 * g + r;
            if (row >= p.tokens) continue;
#pragma unroll
            for (int j = 0; j < NT; ++j) slab[row * n2 + n0 + (wn * NT + j) * 16 + c16] = acc[i][j][r];
        }
}

// a projection value: the slabs added in slab order
__device__ __forceinline__ float slab_sum(const CmpParams &p, int64_t row, int col)
{
    const int64_t n2 = 2 * p.ww, step = p.tokens * n2;
    const float *q = p.slabs + row * n2 + col;
    float v = q[0];
    for (int s = 1; s < p.ksplit; ++s) v += q[s * step];
    return v;
}

// the state_cache row of position pos of sequence b (start = its start_pos), -1 where the table does not name one inside the cache
__device__ __forceinline__ int64_t state_row(const CmpParams &p, int b, int pos, int start)
{
    const int32_t *trow = p.table + (int64_t)b * p.table_stride;
    if (p.cache_mode == 1) {
        const int col = pos / p.block_size;
        if (col >= p.table_cols) return -1;
        const int blk = trow[col];
        if (blk < 0 || blk >= p.state_blocks) return -1;
        return (int64_t)blk * p.block_size + (pos - col * p.block_size);
    }
    const int col = p.coff * p.r + (pos - start);
    if (col < 0 || col >= p.table_cols) return -1;
    const int64_t loc = trow[col];
    return loc >= 0 && loc < p.state_rows ? loc : -1;
}

template <bool BF16>
__global__ __launch_bounds__(512) void compressor_compress_kernel(CmpParams p)
{
    __shared__ float red[8];
    __shared__ float rope[64];
    const int d = threadIdx.x, D = p.d, slot = blockIdx.x;
    uint16_t *orow = p.out + (int64_t)slot * D;
    // ---- the slot's sequence and group
    int b, j;
    if (p.th) {
        int lo = 0, hi = p.batch;      // the last b with group_off[b] <= slot
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p.group_off[mid + 1] <= slot) lo = mid + 1;
            else hi = mid;
        }
        b = lo;
        j = b < p.batch ? slot - p.group_off[b] : 0;
    } else {
        b = slot / p.cg, j = slot % p.cg;
    }
    Seq s{0, 0, 0};
    bool filled = b < p.batch;
    if (filled) {
        s = seq_of(p, b);
        filled = j < groups_of(p, s);
    }
    if (!filled) {      // block-uniform
        orow[d] = 0;
        return;
    }
    const int gs = (s.start / p.r + j) * p.r;      // first position of the group
    const int n2 = 2 * p.ww;
    float m = -INFINITY, l = 0.f, o = 0.f;
    for (int part = 0; part < p.coff; ++part) {
        // coff = 2: the previous group's channels [0, D), then this group's [D, 2 D)
        const int p0 = gs - (p.coff - 1 - part) * p.r, ch = part * D + d;
        for (int i = 0; i < p.r; ++i) {
            const int pos = p0 + i;
            if (pos < 0) continue;      // before the sequence: kv 0, score -inf
            float kv, sc;
            if (pos >= s.start) {
                const int64_t row = s.base + (pos - s.start);
                kv = slab_sum(p, row, ch);
                sc = slab_sum(p, row, p.ww + ch) + p.ape[(pos % p.r) * p.ww + ch];
            } else {
                const int64_t row = state_row(p, b, pos, s.start);
                if (row < 0) continue;
                kv = p.state[row * n2 + ch];
                sc = p.state[row * n2 + p.ww + ch];
            }
            if (sc == -INFINITY) continue;
            const float mn = fmaxf(m, sc);
            const float a = expf(m - mn), e = expf(sc - mn);      // m = -inf: a = 0
            l = l * a + e;
            o = o * a + e * kv;
            m = mn;
        }
    }
    float v = l > 0.f ? o / l : 0.f;
    // ---- RMSNorm over the D channels: wave sums, then the wave sums in wave order
    float sq = v * v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if ((d & 63) == 0) red[d >> 6] = sq;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < D / 64; ++w) tot += red[w];
    v = p.norm_w[d] * (v * (1.0f / sqrtf(tot / (float)D + p.eps)));
    // ---- RoPE on the last 64 channels
    const int e = d - (D - 64);
    if (e >= 0) rope[e] = v;
    __syncthreads();
    if (e >= 0) {
        const float *sn = p.rope_sin + (int64_t)slot * 64, *cs = p.rope_cos + (int64_t)slot * 64;
        if (p.rotary == 1) v = e < 32 ? rope[e] * cs[e] - rope[e + 32] * sn[e] : rope[e - 32] * sn[e] + rope[e] * cs[e];
        else v = (e & 1) ? rope[e - 1] * sn[e] + rope[e] * cs[e] : rope[e] * cs[e] - rope[e + 1] * sn[e];
    }
    orow[d] = cvt_out<BF16>(v);
}

__global__ __launch_bounds__(256) void compressor_save_kernel(CmpParams p)
{
    const int64_t row = blockIdx.x;
    int b, i;
    if (p.th) {
        int lo = 0, hi = p.batch;      // the sequence b with cu[b] <= row < cu[b + 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)p.cu[mid + 1] <= row) lo = mid + 1;
            else hi = mid;
        }
        b = lo;
        if (b >= p.batch) return;
        i = (int)(row - p.cu[b]);
    } else {
        b = (int)(row / p.seq), i = (int)(row % p.seq);
    }
    const Seq s = seq_of(p, b);
    if (i < 0 || i >= s.used) return;
    const int pos = s.start + i;
    if (p.cache_mode == 1) {
        const int col = pos / p.block_size;
        if (col >= p.table_cols || p.table[(int64_t)b * p.table_stride + col] == 0) return;      // block 0 is never written
    } else {
        const int64_t done = ((int64_t)s.start + s.used) / p.r * p.r;      // groups before it are complete
        if ((int64_t)pos / p.r * p.r < done - (int64_t)(p.coff - 1) * p.r) return;
    }
    const int64_t dst = state_row(p, b, pos, s.start);
    if (dst < 0) return;
    const int n2 = 2 * p.ww;
    float *out = p.state + dst * n2;
    const float *ape = p.ape + (pos % p.r) * p.ww;
    for (int c = threadIdx.x; c < n2; c += 256) {
        float v = slab_sum(p, row, c);
        if (c >= p.ww) v += ape[c - p.ww];
        out[c] = v;
    }
}

struct Form {
    bool skinny;
    int ksplit;
};
// the GEMM form and its K split from host integers alone
Form choose_form(int64_t tokens, int ww, int hidden)
{
    Form f;
    f.skinny = tokens <= kSkinnyRows;
    const int64_t tiles = ((tokens + 127) / 128) * (2 * ww / (f.skinny ? 32 : 128));
    const int cu = mi_gqa::cus(), ktiles = hidden / kBK;
    int s = 1;
    while (s < kMaxKSplit && tiles * s * 2 <= cu && ktiles / (s * 2) >= 4) s *= 2;
    f.ksplit = s;
    return f;
}
size_t head_bytes(int batch) { return (((size_t)batch + 1) * sizeof(int32_t) + 255) / 256 * 256; }

bool shape_ok(int r, int coff, int d) { return (r == 4 && coff == 2 && (d == 512 || d == 128)) || (r == 128 && coff == 1 && d == 512); }

}  // namespace
}  // namespace mi_sgl

using namespace mi_sgl;

extern "C" size_t mi_compressor_workspace(int64_t tokens, int batch, int hidden, int head_dim, int coff)
{
    if (tokens <= 0 || batch <= 0 || hidden < 1024 || hidden > 10240 || hidden % 512 || (coff != 1 && coff != 2) ||
        (head_dim != 128 && head_dim != 512))
        return 0;
    const int ww = coff * head_dim;
    return head_bytes(batch) + (size_t)choose_form(tokens, ww, hidden).ksplit * (size_t)tokens * 2 * ww * sizeof(float);
}

extern "C" int mi_compressor(const mi_compressor_params *a, void *stream)
{
    if (!a) return MI_SGL_EINVAL;
    if (!shape_ok(a->cmp_ratio, a->coff, a->head_dim)) return MI_SGL_EINVAL;
    if (a->hidden < 1024 || a->hidden > 10240 || a->hidden % 512) return MI_SGL_EINVAL;
    if (a->rope_head_dim != 64 || (a->rotary_mode != 1 && a->rotary_mode != 2)) return MI_SGL_EINVAL;
    if (a->cache_mode != 1 && a->cache_mode != 2) return MI_SGL_EINVAL;
    if (a->dtype != MI_DTYPE_BF16 && a->dtype != MI_DTYPE_F16) return MI_SGL_EINVAL;
    if (a->layout != MI_COMPRESSOR_TH && a->layout != MI_COMPRESSOR_BSH) return MI_SGL_EINVAL;
    if (a->table_dims != 1 && a->table_dims != 2) return MI_SGL_EINVAL;
    if (a->cache_mode == 2 && (a->table_dims != 2 || a->table_cols < a->coff * a->cmp_ratio + 1)) return MI_SGL_EINVAL;
    if (a->state_blocks < 1 || a->block_size < 1 || a->table_cols < 1) return MI_SGL_EINVAL;
    const int ww = a->coff * a->head_dim;
    if (a->state_cache_stride_dim0 != 0 && a->state_cache_stride_dim0 != (int64_t)a->block_size * 2 * ww) return MI_SGL_EINVAL;
    if (!(a->norm_eps >= 0.f) || !(a->norm_eps < INFINITY)) return MI_SGL_EINVAL;
    const bool th = a->layout == MI_COMPRESSOR_TH;
    if (a->batch < 0 || a->tokens < 0 || (!th && (a->seq < 0 || a->tokens != (int64_t)a->batch * a->seq))) return MI_SGL_EINVAL;
    if (a->tokens > INT32_MAX / 2 || a->state_blocks * a->block_size > INT32_MAX) return MI_SGL_EINVAL;
    const int cg = th ? 0 : (a->seq + a->cmp_ratio - 1) / a->cmp_ratio;
    const int64_t out_rows = th ? (a->tokens < a->tokens / a->cmp_ratio + a->batch ? a->tokens : a->tokens / a->cmp_ratio + a->batch)
                                : (int64_t)a->batch * cg;
    if (a->out_rows != out_rows) return MI_SGL_EINVAL;
    if (a->tokens == 0 || a->batch == 0) return MI_SGL_OK;
    if (!a->x || !a->wkv || !a->wgate || !a->state_cache || !a->ape || !a->norm_weight || !a->rope_sin || !a->rope_cos ||
        !a->state_block_table || !a->cmp_kv || !a->workspace || (th && !a->cu_seqlens) || (!th && a->cu_seqlens))
        return MI_SGL_EINVAL;
    const Form form = choose_form(a->tokens, ww, a->hidden);
    const size_t head = head_bytes(a->batch);
    if (a->workspace_bytes < head + (size_t)form.ksplit * (size_t)a->tokens * 2 * ww * sizeof(float)) return MI_SGL_EINVAL;

    CmpParams p;
    p.x = (const uint16_t *)a->x, p.wkv = (const uint16_t *)a->wkv, p.wgate = (const uint16_t *)a->wgate;
    p.state = a->state_cache, p.ape = a->ape, p.norm_w = a->norm_weight, p.rope_sin = a->rope_sin, p.rope_cos = a->rope_cos;
    p.table = a->state_block_table, p.cu = a->cu_seqlens, p.seqused = a->seqused, p.start_pos = a->start_pos;
    p.out = (uint16_t *)a->cmp_kv;
    p.group_off = (int32_t *)a->workspace, p.slabs = (float *)((uint8_t *)a->workspace + head);
    p.tokens = a->tokens, p.out_rows = out_rows, p.state_rows = a->state_blocks * a->block_size;
    p.batch = a->batch, p.seq = th ? 0 : a->seq, p.th = th, p.hidden = a->hidden, p.d = a->head_dim, p.ww = ww, p.r = a->cmp_ratio;
    p.coff = a->coff, p.rotary = a->rotary_mode, p.cache_mode = a->cache_mode, p.block_size = a->block_size;
    p.table_cols = a->table_dims == 2 ? a->table_cols : 1, p.table_stride = a->table_dims == 2 ? a->table_stride : 1;
    p.ksplit = form.ksplit, p.cg = cg > 0 ? cg : 1, p.state_blocks = a->state_blocks, p.eps = a->norm_eps;

    hipStream_t st = (hipStream_t)stream;
    const bool bf16 = a->dtype == MI_DTYPE_BF16;
    constexpr size_t lds_large = 2 * (128 + 128) * kRowBytes, lds_skinny = 4 * (128 + 32) * kRowBytes;
    static PerDeviceOnce attr_once;
    if (attr_once.need()) {
        (void)hipFuncSetAttribute((const void *)compressor_gemm_kernel<true, 2, 2, 4, 4, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_large);
        (void)hipFuncSetAttribute((const void *)compressor_gemm_kernel<false, 2, 2, 4, 4, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_large);
        (void)hipFuncSetAttribute((const void *)compressor_gemm_kernel<true, 4, 1, 2, 2, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_skinny);
        (void)hipFuncSetAttribute((const void *)compressor_gemm_kernel<false, 4, 1, 2, 2, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_skinny);
    }
    compressor_plan_kernel<<<1, kPlanThreads, 0, st>>>(p);
    const int64_t mt = (a->tokens + 127) / 128;
    if (form.skinny) {
        const dim3 grid((unsigned)(mt * form.ksplit * (2 * ww / 32)));
        if (bf16) compressor_gemm_kernel<true, 4, 1, 2, 2, 4><<<grid, 256, lds_skinny, st>>>(p);
        else compressor_gemm_kernel<false, 4, 1, 2, 2, 4><<<grid, 256, lds_skinny, st>>>(p);
    } else {
        const dim3 grid((unsigned)(mt * form.ksplit * (2 * ww / 128)));
        if (bf16) compressor_gemm_kernel<true, 2, 2, 4, 4, 2><<<grid, 256, lds_large, st>>>(p);
        else compressor_gemm_kernel<false, 2, 2, 4, 4, 2><<<grid, 256, lds_large, st>>>(p);
    }
    if (bf16) compressor_compress_kernel<true><<<(unsigned)out_rows, a->head_dim, 0, st>>>(p);
    else compressor_compress_kernel<false><<<(unsigned)out_rows, a->head_dim, 0, st>>>(p);
    compressor_save_kernel<<<(unsigned)a->tokens, 256, 0, st>>>(p);
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}
