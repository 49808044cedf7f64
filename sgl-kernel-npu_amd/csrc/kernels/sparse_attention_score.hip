// Block-sparse grouped-query attention over per-token block lists for gfx950: torch.ops.npu.npu_sparse_attention_score, the reference's
// native main-attention op (csrc/sparse_attention_score/: op_host/sparse_attention_score.cpp, op_kernel/arch35/
// sparse_attention_score_kernel_arch35.h:112-163 and ..._arch35_full_quant.h:139-302).  query [T, Hq, D] in TND layout, K / V caches
// [pages, block_size, Hkv, D], select_idx [Hkv, Q, topK] logical block ids of which the first select_num_idx[kh, t] are live, a block table
// [batch, columns], per-request query and kv lengths.  Token t is token j of the request b whose running sum of query lengths covers it and
// stands at pos = kv_len[b] - q_len[b] + j: it sees the keys of its live blocks at logical positions <= pos.
//
// The structure is gqa_sparse_decode.hip's (the engine is gqa_common.h's tile_step: S^T = K.Q^T and O^T += V^T.P^T on the MFMA, online
// softmax in the log2 domain, 64-key tiles double buffered in LDS with the padded row stride): a workgroup of 4 waves owns one (token, kv
// head, chunk of the list) and all query heads of the group, resolves the chunk's live slots ONCE into an LDS list (logical block, page)
// and cuts the chunk's slots x block_size keys into 64-key tiles.  With seq_len = pos + 1 the causal end of a token is the sequence end of
// that kernel.  What is new: every wave finds (b, j) by a prefix scan of the query lengths across its lanes; the live prefix of the list;
// and the FP8 (e4m3fn) form, which loads 1-byte elements, converts them to fp16 (exact) on the way into LDS and runs the fp16 engine -- the
// block's k scale times the head's q scale multiplies the scores before the mask, the block's v scale is folded into the staged V rows
// (v8 * sv rounded to fp16).  Chunks write fp32 partials that gqa_common.h's merge kernel combines.  The chunk count comes from shapes and
// the CU count only: nothing is read back, the launches can be captured in a graph.
#include <algorithm>

#include "device_once.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gqa_common.h"
#include "mi_sgl_kernels.h"

namespace mi_sparse_score {
using namespace mi_gqa;

constexpr int kTile = 64;
constexpr int kMaxTopk = 1024;      // list entries of a token; a chunk keeps its share in LDS (8 B each, 16 B with FP8 scales)

struct Params {
    const void *q, *k, *v;          // 2-byte elements, or 1-byte e4m3fn
    uint16_t *out;
    const int32_t *sel, *sel_num, *table, *q_lens, *kv_lens;
    const float *q_scale, *k_scale, *v_scale;      // [batch, q_heads, q_scale_blocks], [batch, kv_heads, columns] twice; FP8 only
    float *ws_o, *ws_ml;            // [T][Hq][chunks][DP] unnormalised partial outputs; [T][Hq][chunks][2] running max (log2 domain), sum
    int tokens, batch, q_heads, kv_heads, group, block_size, bs_shift, topk_n, columns, num_pages, q_scale_blocks, num_chunks, chunk_slots,
        list_cap, d;
    int64_t q_st, q_sh, k_sblk, k_srow, k_sh, v_sblk, v_srow, v_sh, o_st, o_sh, sel_sh, sel_sq, sel_sk, num_sh, num_sq, tb_sb, tb_sn;
    float sm_scale;
};

// Where token t stands: request b, position pos (-1 = the token lies behind the sum of the query lengths, or before position 0).  Every
// wave does this for itself, without LDS or a barrier: lane l sums the lengths of requests [l per, (l + 1) per), an inclusive scan across the
// lanes (DPP row shifts and broadcasts) finds the first lane whose sum passes t, and that lane walks its requests.  Lengths below zero count
// as zero; sums saturate at 2^31 - 1 > t, which no comparison with t can tell from the true sum.
__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) { return min(a + b, 0x7fffffffu); }      // a, b <= 2^31 - 1: no wrap
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t x)      // lanes the pattern gives no source, or the row mask leaves out, read 0
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ void locate_token(const Params &p, int t, int lane, int &b_out, int &pos_out)
{
    if (!p.q_lens) {                                              // one token per request
        b_out = t < p.batch ? t : 0;
        pos_out = t < p.batch ? max(p.kv_lens[b_out], 0) - 1 : -1;
        return;
    }
    // a lane's first kInReg requests -- all of them up to a batch of 256 -- are loaded once, lengths of both kinds together, so that nothing
    // is loaded behind the scan (batch >= 1 here: the entry point launches nothing for an empty batch)
    constexpr int kInReg = 4;
    const int per = (p.batch + 63) >> 6, r0 = lane * per, r1 = min(p.batch, r0 + per);
    int ql[kInReg], kl[kInReg];
#pragma unroll
    for (int k = 0; k < kInReg; ++k) {                            // every load at an index inside the vectors, none behind a branch
        const int i = min(r0 + k, p.batch - 1);
        const int qv = p.q_lens[i], kv = p.kv_lens[i];
        const bool in = k < per && r0 + k < r1;
        ql[k] = in ? max(qv, 0) : 0, kl[k] = in ? kv : 0;
    }
    uint32_t incl = 0;
#pragma unroll
    for (int k = 0; k < kInReg; ++k) incl = sat_add(incl, (uint32_t)ql[k]);
    for (int i = r0 + kInReg; i < r1; ++i) incl = sat_add(incl, (uint32_t)max(p.q_lens[i], 0));
    incl = sat_add(incl, dpp_or_zero<0x111, 0xf>(incl));          // row_shr:1, 2, 4, 8: the scan inside every row of 16 lanes
    incl = sat_add(incl, dpp_or_zero<0x112, 0xf>(incl));
    incl = sat_add(incl, dpp_or_zero<0x114, 0xf>(incl));
    incl = sat_add(incl, dpp_or_zero<0x118, 0xf>(incl));
    incl = sat_add(incl, dpp_or_zero<0x142, 0xa>(incl));          // row_bcast:15 into rows 1 and 3: the total of the row before
    incl = sat_add(incl, dpp_or_zero<0x143, 0xc>(incl));          // row_bcast:31 into rows 2 and 3: the total of rows 0 and 1
    const unsigned long long covers = __ballot((uint32_t)t < incl);      // the sums do not decrease: every lane from the owner on
    int b = 0, pos = -1;
    if (covers) {
        const int owner = __builtin_ctzll(covers);
        uint32_t run = owner ? (uint32_t)__builtin_amdgcn_readlane((int)incl, owner - 1) : 0u;      // <= t: not saturated
        if (lane == owner) {
            bool found = false;
            auto visit = [&](int i, int len, int kv) {            // request i of this lane's range: does it hold token t?
                if (found) return;
                if ((uint32_t)t < sat_add(run, (uint32_t)len)) {
                    const long long at = (long long)kv - len + (long long)((uint32_t)t - run);
                    b = i, pos = at < 0 ? -1 : (int)min(at, (long long)0x7ffffffe), found = true;
                } else {
                    run += (uint32_t)len;
                }
            };
#pragma unroll
            for (int k = 0; k < kInReg; ++k)
                if (r0 + k < r1) visit(r0 + k, ql[k], kl[k]);
            for (int i = r0 + kInReg; i < r1 && !found; ++i) visit(i, max(p.q_lens[i], 0), p.kv_lens[i]);
        }
        b = __builtin_amdgcn_readlane(b, owner), pos = __builtin_amdgcn_readlane(pos, owner);
    }
    b_out = b, pos_out = pos;
}

// 4 e4m3fn bytes -> 4 fp32 (exact)
__device__ __forceinline__ void fp8x4_to_f32(uint32_t w, float (&f)[4])
{
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    f[0] = lo[0], f[1] = lo[1], f[2] = hi[0], f[3] = hi[1];
}
// 8 e4m3fn bytes (two words) times `scale`, rounded to fp16: 16 bytes of an LDS row
__device__ __forceinline__ u32x4 fp8x8_to_f16(uint32_t w0, uint32_t w1, float scale)
{
    float a[4], c[4];
    fp8x4_to_f32(w0, a), fp8x4_to_f32(w1, c);
    return u32x4{pack2<false>(a[0] * scale, a[1] * scale), pack2<false>(a[2] * scale, a[3] * scale), pack2<false>(c[0] * scale, c[1] * scale),
                 pack2<false>(c[2] * scale, c[3] * scale)};
}

// DP: compile-time padded head dim (64, 128, 256); HB head blocks of 16 per wave (a workgroup covers 64 * HB heads of the group); FP8: 1-byte
// q / k / v with dequantisation scales, fp16 engine and output (BF16 = false, DP = 128).
template <bool BF16, bool FP8, int DP, int HB>
__global__ __launch_bounds__(256) void sparse_attention_score_kernel(Params p)
{
    constexpr int TILE = kTile, KS = row_stride(DP), kBuf = TILE * 2 * KS;
    constexpr int MT = TILE / 16, QS = DP / 32, DT = DP / 16;
    // staging: 8 threads per row, 32 rows a pass; a thread moves 16 bytes of the row per load -- 8 two-byte elements (one 16-B LDS chunk),
    // or 16 one-byte elements (two LDS chunks)
    constexpr int C = DP / 8, RP = TILE / 32, J = FP8 ? (C + 15) / 16 : (C + 7) / 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    int32_t *s_lb = (int32_t *)(lds + 2 * kBuf), *s_pg = s_lb + p.list_cap;
    float *s_sk = (float *)(s_pg + p.list_cap), *s_sv = s_sk + p.list_cap;      // FP8 only (the launch sizes LDS for them then)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    constexpr int kHeadsPerWg = 64 * HB;
    const int head_blocks = (p.group + kHeadsPerWg - 1) / kHeadsPerWg;
    int u = blockIdx.x;                                           // the grid is exactly tokens * kv_heads * chunks * head_blocks
    const int hblk = u % head_blocks;
    u /= head_blocks;
    const int chunk = u % p.num_chunks;
    u /= p.num_chunks;
    const int kvh = u % p.kv_heads, t_tok = u / p.kv_heads;
    const int BS = p.block_size, shift = p.bs_shift;

    // the count and this thread's first slot do not depend on where the token stands: their loads travel with locate_token's
    const int s_begin = chunk * p.chunk_slots;
    const int n_raw = p.sel_num ? p.sel_num[kvh * p.num_sh + t_tok * p.num_sq] : p.topk_n;
    const int32_t *sel_row = p.sel + kvh * p.sel_sh + t_tok * p.sel_sq;
    const int32_t first_id = (tid < p.chunk_slots && s_begin + tid < p.topk_n) ? sel_row[(int64_t)(s_begin + tid) * p.sel_sk] : -1;
    int b, pos;
    locate_token(p, t_tok, lane, b, pos);
    const int qblk = pos >> shift;                                // the diagonal block; with FP8 also the column of the token's q scale
    const bool live = pos >= 0 && (!FP8 || qblk < p.q_scale_blocks);
    const int seq_len = live ? pos + 1 : 0;                       // keys at logical positions < seq_len take part

    // ---- the chunk's live slots -> (logical block, page); -1 for a slot that names no block, one behind the diagonal block, one outside the
    // table (its entry is not read) or one whose page lies outside the cache.  What a slot behind the live prefix holds is never used as a
    // block id (a thread's first slot is loaded before the count is known and dropped when it lies behind it).
    const int n_live = live ? min(max(n_raw, 0), p.topk_n) : 0;
    const int n_slots = max(0, min(n_live, s_begin + p.chunk_slots) - s_begin);
    for (int i = tid; i < p.list_cap; i += 256) {
        int32_t lb = -1, pg = 0;
        float sk = 0.f, sv = 0.f;
        if (i < n_slots) {
            const int32_t l = i == tid ? first_id : sel_row[(int64_t)(s_begin + i) * p.sel_sk];
            if (l >= 0 && l <= qblk && l < p.columns) {
                const int32_t page = p.table[b * p.tb_sb + l * p.tb_sn];
                if constexpr (FP8) {                              // beside the table's entry, not behind it
                    const int64_t at = ((int64_t)b * p.kv_heads + kvh) * p.columns + l;
                    sk = p.k_scale[at], sv = p.v_scale[at];
                }
                if (page >= 0 && page < p.num_pages) lb = l, pg = page;
                else sk = 0.f, sv = 0.f;                          // a dropped slot keeps no scale: whatever it held multiplies nothing
            }
        }
        s_lb[i] = lb, s_pg[i] = pg;
        if constexpr (FP8) s_sk[i] = sk, s_sv[i] = sv;
    }

    // Q^T fragments: lane (g, c16) holds q[head][ks*32 + g*8 .. +8] of head block hb
    s16x8 qf[HB][QS];
    int hg[HB];
    bool wave_has[HB];
    f32x4 acc[HB][DT];
    float m_run[HB], l_run[HB], sq[HB];
    const float cs = p.sm_scale * 1.4426950408889634f;
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        hg[hb] = hblk * kHeadsPerWg + (hb * 4 + wave) * 16 + c16;
        wave_has[hb] = hblk * kHeadsPerWg + (hb * 4 + wave) * 16 < p.group;      // waves without a real head still help to stage tiles
        const bool ok = hg[hb] < p.group;
        const int head = kvh * p.group + (hg[hb] < p.group ? hg[hb] : 0);
        sq[hb] = 1.f;
        if constexpr (FP8) {
            const uint8_t *qrow = (const uint8_t *)p.q + (int64_t)t_tok * p.q_st + (int64_t)head * p.q_sh;
            if (ok && live) sq[hb] = p.q_scale[((int64_t)b * p.q_heads + head) * p.q_scale_blocks + qblk];
#pragma unroll
            for (int ks = 0; ks < QS; ++ks) {
                const int d = ks * 32 + g * 8;
                const uint2 w = (ok && d < p.d) ? *(const uint2 *)(qrow + d) : uint2{0u, 0u};
                qf[hb][ks] = __builtin_bit_cast(s16x8, fp8x8_to_f16(w.x, w.y, 1.f));
            }
        } else {
            const uint16_t *qrow = (const uint16_t *)p.q + (int64_t)t_tok * p.q_st + (int64_t)head * p.q_sh;
#pragma unroll
            for (int ks = 0; ks < QS; ++ks) {
                const int d = ks * 32 + g * 8;
                qf[hb][ks] = (ok && d < p.d) ? *(const s16x8 *)(qrow + d) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
        m_run[hb] = -INFINITY, l_run[hb] = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i) acc[hb][i] = f32x4{0.f, 0.f, 0.f, 0.f};
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
                any |= lb >= 0 && (int64_t)lb * BS + n0 < seq_len;
            }
            if (any) break;
        }
        return t;
    };

    u32x4 kreg[RP][J], vreg[RP][J];
    float svreg[RP];
    const int srow = tid >> 3, sch = tid & 7;
    auto stage_load = [&](int tile) {
#pragma unroll
        for (int rp = 0; rp < RP; ++rp) {
            const int j = tile * TILE + rp * 32 + srow, slot = j >> shift, n = j & (BS - 1);
            const int lb = s_lb[slot];
            const int64_t pg = s_pg[slot];
            const bool ok = lb >= 0 && (int64_t)lb * BS + n < seq_len;      // rows that take no part are zeros in LDS and are never read from the caches
            if constexpr (FP8) {
                svreg[rp] = ok ? s_sv[slot] : 0.f;                 // rows that take no part are 0 * 0, whatever the block's scale holds
                const uint8_t *kr = (const uint8_t *)p.k + pg * p.k_sblk + (int64_t)n * p.k_srow + (int64_t)kvh * p.k_sh;
                const uint8_t *vr = (const uint8_t *)p.v + pg * p.v_sblk + (int64_t)n * p.v_srow + (int64_t)kvh * p.v_sh;
#pragma unroll
                for (int jj = 0; jj < J; ++jj) {
                    const int c = sch + 8 * jj;                   // 16 elements from c * 16
                    const bool in = ok && c * 16 < p.d;
                    kreg[rp][jj] = in ? *(const u32x4 *)(kr + c * 16) : u32x4{0, 0, 0, 0};
                    vreg[rp][jj] = in ? *(const u32x4 *)(vr + c * 16) : u32x4{0, 0, 0, 0};
                }
            } else {
                const uint16_t *kr = (const uint16_t *)p.k + pg * p.k_sblk + (int64_t)n * p.k_srow + (int64_t)kvh * p.k_sh;
                const uint16_t *vr = (const uint16_t *)p.v + pg * p.v_sblk + (int64_t)n * p.v_srow + (int64_t)kvh * p.v_sh;
#pragma unroll
                for (int jj = 0; jj < J; ++jj) {
                    const int c = sch + 8 * jj;
                    const bool in = ok && c * 8 < p.d;
                    kreg[rp][jj] = in ? *(const u32x4 *)(kr + c * 8) : u32x4{0, 0, 0, 0};
                    vreg[rp][jj] = in ? *(const u32x4 *)(vr + c * 8) : u32x4{0, 0, 0, 0};
                }
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
                if constexpr (FP8) {
                    if (c * 2 < C) {                              // 16 elements: LDS chunks 2c and 2c + 1
                        uint8_t *kd = buf + row * KS + c * 32, *vd = kd + TILE * KS;
                        const u32x4 kw = kreg[rp][jj], vw = vreg[rp][jj];
                        *(u32x4 *)kd = fp8x8_to_f16(kw[0], kw[1], 1.f);
                        *(u32x4 *)(kd + 16) = fp8x8_to_f16(kw[2], kw[3], 1.f);
                        *(u32x4 *)vd = fp8x8_to_f16(vw[0], vw[1], svreg[rp]);
                        *(u32x4 *)(vd + 16) = fp8x8_to_f16(vw[2], vw[3], svreg[rp]);
                    }
                } else {
                    if (c < C) {
                        *(u32x4 *)(buf + row * KS + c * 16) = kreg[rp][jj];
                        *(u32x4 *)(buf + TILE * KS + row * KS + c * 16) = vreg[rp][jj];
                    }
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
            const float sq_h = sq[hb];
            tile_step<BF16, DP, DP, TILE>(buf, qf[hb], acc[hb], m_run[hb], l_run[hb], cs, g, c16, [&](f32x4(&s)[MT]) {
                // 16 keys of an MFMA row block lie in one block (BS >= 16): keys r < lim of this lane's four take part
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int j0 = t * TILE + mt * 16, slot = j0 >> shift;
                    const int lb = s_lb[slot];
                    const int64_t left = lb < 0 ? 0 : (int64_t)seq_len - (int64_t)lb * BS - ((j0 & (BS - 1)) + 4 * g);
                    const int lim = (int)min(left, (int64_t)4);
                    if constexpr (FP8) {                          // dequantise first: a scale of 0 must not meet -inf
                        const float f = sq_h * s_sk[slot];
#pragma unroll
                        for (int r = 0; r < 4; ++r) s[mt][r] *= f;
                    }
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
            const float inv = l_run[hb] > 0.f ? 1.f / l_run[hb] : 0.f;      // no key at all: zeros
            uint16_t *orow = p.out + (int64_t)t_tok * p.o_st + (int64_t)head * p.o_sh + 4 * g;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (dt * 16 + 4 * g >= p.d) continue;             // d % 8 == 0: the 4 dims are in or out together
                const uint32_t w0 = pack2<BF16>(acc[hb][dt][0] * inv, acc[hb][dt][1] * inv);
                const uint32_t w1 = pack2<BF16>(acc[hb][dt][2] * inv, acc[hb][dt][3] * inv);
                *(uint2 *)(orow + dt * 16) = uint2{w0, w1};
            }
        } else {
            const int64_t idx = ((int64_t)t_tok * p.q_heads + head) * p.num_chunks + chunk;
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

template <bool BF16, bool FP8, int DP, int HB>
static void launch_one(const Params &p, unsigned grid, hipStream_t st)
{
    constexpr size_t tiles = 2 * (size_t)kTile * 2 * row_stride(DP), per_slot = (FP8 ? 4 : 2) * sizeof(int32_t);
    static PerDeviceOnce attr_once;
    if (attr_once.need()) {
        (void)hipFuncSetAttribute((const void *)sparse_attention_score_kernel<BF16, FP8, DP, HB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(tiles + per_slot * kMaxTopk));
    }
    sparse_attention_score_kernel<BF16, FP8, DP, HB><<<grid, 256, tiles + per_slot * p.list_cap, st>>>(p);
}

}  // namespace mi_sparse_score

using namespace mi_sparse_score;

extern "C" size_t mi_sparse_attention_score_workspace(int64_t tokens, int q_heads, int head_dim, int num_chunks)
{
    const int dp = padded_dim(head_dim);
    if (tokens <= 0 || q_heads <= 0 || head_dim <= 0 || !dp || num_chunks <= 1) return 0;
    return (size_t)tokens * q_heads * num_chunks * (dp + 2) * sizeof(float);
}

// Chunks of the list per (token, kv head): mi_gqa_sparse_decode_num_chunks' rule with tokens in the place of sequences -- a power of two
// that brings the grid to about two workgroups per CU, at most the list's length and 64.  From shapes and the CU count only.
extern "C" int mi_sparse_attention_score_num_chunks(int64_t tokens, int kv_heads, int topk)
{
    if (tokens <= 0 || kv_heads <= 0 || topk <= 1) return 1;
    const long long wgs = (long long)tokens * kv_heads;
    const long long want = std::min<long long>(std::min<long long>((2ll * cus() + wgs - 1) / wgs, topk), 64);
    int c = 1;
    while (2 * c <= want) c *= 2;
    return c;
}

extern "C" int mi_sparse_attention_score(const mi_sparse_attention_score_params *a, void *stream)
{
    if (!a) return MI_SGL_EINVAL;
    const bool fp8 = a->dtype == MI_DTYPE_FP8_E4M3;
    if (a->tokens < 0 || a->tokens > 0x7fffffffll || a->batch < 0 || a->q_heads <= 0 || a->kv_heads <= 0 || a->q_heads % a->kv_heads) return MI_SGL_EINVAL;
    if (a->topk < 1 || a->topk > kMaxTopk || a->columns < 0 || a->num_pages < 0) return MI_SGL_EINVAL;
    if (!block_args_ok(a->block_size, a->head_dim, fp8 ? MI_DTYPE_F16 : a->dtype, a->sm_scale)) return MI_SGL_EINVAL;
    if (fp8 && (a->head_dim != 128 || a->block_size != 128 || a->q_scale_blocks < 1)) return MI_SGL_EINVAL;
    const int dp = padded_dim(a->head_dim);
    int num_chunks = a->num_chunks;
    if (num_chunks == 0) num_chunks = mi_sparse_attention_score_num_chunks(a->tokens, a->kv_heads, a->topk);
    if (num_chunks < 0 || num_chunks > a->topk) return MI_SGL_EINVAL;
    if (a->tokens == 0 || a->batch == 0) return MI_SGL_OK;
    if (!a->q || !a->k || !a->v || !a->out || !a->select_idx || !a->block_table || !a->actual_seq_lengths_kv) return MI_SGL_EINVAL;
    if (!a->actual_seq_lengths && a->tokens != a->batch) return MI_SGL_EINVAL;
    if (fp8 != (a->q_dequant_scale != nullptr) || fp8 != (a->k_dequant_scale != nullptr) || fp8 != (a->v_dequant_scale != nullptr)) return MI_SGL_EINVAL;
    // 16-byte loads of the cache rows (8 two-byte or 16 one-byte elements), 16- / 8-byte loads of the query rows, 8-byte stores
    const int64_t in_align = fp8 ? 16 : 8;
    for (const int64_t s : {a->k_stride_blk, a->k_stride_row, a->k_stride_h, a->v_stride_blk, a->v_stride_row, a->v_stride_h})
        if (s % in_align) return MI_SGL_EINVAL;
    if ((a->q_stride_t % 8) || (a->q_stride_h % 8) || (a->o_stride_t % 4) || (a->o_stride_h % 4)) return MI_SGL_EINVAL;
    if (((uintptr_t)a->q & (fp8 ? 7 : 15)) || ((uintptr_t)a->k & 15) || ((uintptr_t)a->v & 15) || ((uintptr_t)a->out & 7)) return MI_SGL_EINVAL;
    if (num_chunks > 1 && (!a->workspace || ((uintptr_t)a->workspace & 15) ||
                           a->workspace_bytes < mi_sparse_attention_score_workspace(a->tokens, a->q_heads, a->head_dim, num_chunks)))
        return MI_SGL_EINVAL;
    Params p;
    p.q = a->q, p.k = a->k, p.v = a->v, p.out = (uint16_t *)a->out;
    p.sel = a->select_idx, p.sel_num = a->select_num_idx, p.table = a->block_table, p.q_lens = a->actual_seq_lengths, p.kv_lens = a->actual_seq_lengths_kv;
    p.q_scale = a->q_dequant_scale, p.k_scale = a->k_dequant_scale, p.v_scale = a->v_dequant_scale;
    p.ws_o = (float *)a->workspace;
    p.ws_ml = p.ws_o ? p.ws_o + (size_t)a->tokens * a->q_heads * num_chunks * dp : nullptr;
    p.tokens = (int)a->tokens, p.batch = a->batch, p.q_heads = a->q_heads, p.kv_heads = a->kv_heads, p.group = a->q_heads / a->kv_heads;
    p.block_size = a->block_size, p.bs_shift = __builtin_ctz(a->block_size), p.topk_n = a->topk, p.columns = a->columns, p.num_pages = a->num_pages;
    p.q_scale_blocks = a->q_scale_blocks, p.num_chunks = num_chunks, p.chunk_slots = (a->topk + num_chunks - 1) / num_chunks;
    p.list_cap = (p.chunk_slots + 3) / 4 * 4, p.d = a->head_dim;
    p.q_st = a->q_stride_t, p.q_sh = a->q_stride_h, p.k_sblk = a->k_stride_blk, p.k_srow = a->k_stride_row, p.k_sh = a->k_stride_h;
    p.v_sblk = a->v_stride_blk, p.v_srow = a->v_stride_row, p.v_sh = a->v_stride_h, p.o_st = a->o_stride_t, p.o_sh = a->o_stride_h;
    p.sel_sh = a->idx_stride_h, p.sel_sq = a->idx_stride_q, p.sel_sk = a->idx_stride_k, p.num_sh = a->num_stride_h, p.num_sq = a->num_stride_q;
    p.tb_sb = a->bt_stride_b, p.tb_sn = a->bt_stride_n;
    p.sm_scale = a->sm_scale;
    const int hpw = p.group <= 64 ? 64 : 128;
    const int head_blocks = (p.group + hpw - 1) / hpw;
    const long long wgs = (long long)a->tokens * a->kv_heads * num_chunks * head_blocks;
    if (wgs > 0x7fffffffll) return MI_SGL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool bf16 = a->dtype == MI_DTYPE_BF16;
    if (fp8) {
        if (hpw == 64) launch_one<false, true, 128, 1>(p, (unsigned)wgs, st);
        else launch_one<false, true, 128, 2>(p, (unsigned)wgs, st);
    } else {
        dispatch(bf16, dp, hpw == 64, [&](auto bf, auto d, auto one) { launch_one<bf(), false, d(), one() ? 1 : 2>(p, (unsigned)wgs, st); });
    }
    if (num_chunks > 1) {
        GqaParams m{};                                            // the merge kernel of gqa_common.h on this kernel's partial layout, a token per row
        m.out = (uint16_t *)a->out, m.ws_o = p.ws_o, m.ws_ml = p.ws_ml, m.batch = (int)a->tokens, m.q_heads = a->q_heads, m.kv_heads = a->kv_heads;
        m.group = p.group, m.num_splits = num_chunks, m.lv = a->head_dim, m.o_sb = a->o_stride_t, m.o_sh = a->o_stride_h;
        m.plan = nullptr, m.sinks = nullptr, m.window = -1, m.bt_rows = nullptr;
        const int blocks = (int)(((long long)a->tokens * a->q_heads + 3) / 4);
        if (bf16) gqa_merge_kernel<true><<<blocks, 256, 0, st>>>(m, dp);
        else gqa_merge_kernel<false><<<blocks, 256, 0, st>>>(m, dp);
    }
    return hipGetLastError() == hipSuccess ? MI_SGL_OK : MI_SGL_ELAUNCH;
}
