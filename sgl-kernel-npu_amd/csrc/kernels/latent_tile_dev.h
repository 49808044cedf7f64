// The tile engine of the 64-head latent kernels (mla_decode.hip: paged MLA decode, nope + rope; sparse_sharedkv.hip: window + token-sparse
// attention over one shared latent, no rope).  Both run a workgroup of 4 waves, one per SIMD, 16 heads per wave (lane (g, c16): head c16 of
// the wave, lane group g = lane >> 4), all 512 output dims per wave, over tiles of kTile = 64 keys whose 1-KiB nope rows sit kNopeStride bytes
// apart in LDS.  What a wave does with one tile exists here once:
//   fill     issue_nope_row: one row by LDS-DMA from an address another lane holds; the callers trickle the rows of tile t + 1 in behind
//            the QK MFMAs of tile t
//   QK       qk_scores: S^T[key, head] = K . Q^T, operands kAhead k-steps ahead of their MFMAs
//   softmax  softmax_step: scaled log2 domain, deferred rescale, P packed to the KV dtype in the S^T accumulator layout (= the B operand of P.V)
//   P.V      pv_accumulate: O^T[d, head] += V^T . P^T through the LDS transpose read
//   finish   store_head_out / store_head_partial
// The addressing (which row is a key's), the masks, the start values of (m, l) and which tiles are skipped belong to each kernel.
#pragma once
#include "mla_common.h"

namespace mi_sgl {

// Reductions across the four 16-lane rows of a wave through the permlane swaps (VALU) instead of ds_bpermute (an LDS round trip each).
// swap16(x): {rows 0,0,2,2 | rows 1,1,3,3} of x; swap32(x): {lower half twice | upper half twice}.  Sums and maxima of the two parts are the
// xor-16 / xor-32 butterfly steps (same two operands in every lane: bit-identical to the shuffle form).
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

// LDS-DMA through inline asm: lane l moves 16 B from its own address to dst + 16 l (M0 = wave-uniform LDS destination), 1 KiB per
// wave-instruction.  With the builtin the compiler put an `s_waitcnt vmcnt(0)` behind EVERY piece (it cannot tell which later ds_read the DMA
// might feed), i.e. one memory round trip per QK k-step; the only wait these requests need is the explicit one at the top of the tile loop.
// The compiler's own waits (block-table loads, Q^T) stay correct: requests complete in order, so extra ones in flight only make them
// conservative.
__device__ __forceinline__ void dma_row(const uint8_t *dst_lds, const void *vaddr)
{
    const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)dst_lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(dst), "v"(vaddr) : "memory");
}

// Nope row `row` (wave-uniform) of a tile into `buf`: lane `row` holds the row's byte address in `addr`; two readlanes broadcast it, so no
// vector-memory wait separates consecutive DMA instructions.  A wave contributes rows wave + 4 idx, idx = 0..15.
__device__ __forceinline__ void issue_nope_row(int64_t addr, int row, uint8_t *buf, int lane)
{
    const int lo = __builtin_amdgcn_readlane((int)(addr & 0xFFFFFFFFll), row);
    const int hi = __builtin_amdgcn_readlane((int)(addr >> 32), row);
    const uint8_t *src = (const uint8_t *)(uintptr_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    dma_row(buf + row * kNopeStride, src + lane * 16);
}

// The A operand of QK for the nope dims: keys mt*16 + c16 of the tile, dims ks*32 + g*8 .. +8
__device__ __forceinline__ s16x8 lda_nope(const uint8_t *buf, int ks, int mt, int g, int c16)
{
    return *(const s16x8 *)(buf + (mt * 16 + c16) * kNopeStride + ks * 64 + g * 16);
}

// S^T[key, head] = K . Q^T: 4 m-tiles of 16 keys, KSTEPS k-steps of 32 dims; qf = the wave's resident Q^T fragments, lda(ks, mt) = the A
// operand.  Explicit software pipeline, fenced with sched_barrier so the machine scheduler cannot sink the prefetch back next to its use:
// operands of k-step ks + kAhead are issued before the MFMAs of k-step ks (a ring of kAhead + 1 operand sets).  under(ks) runs behind the
// MFMAs of k-step ks: the place where the fill of the next tile trickles in, one DMA per k-step.
template <bool BF16, int KSTEPS, class LoadA, class Under>
__device__ __forceinline__ void qk_scores(LoadA lda, const s16x8 (&qf)[KSTEPS], f32x4 (&s)[4], Under under)
{
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) s[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int kAhead = 3;
    s16x8 af[kAhead + 1][4];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pre = 0; pre < kAhead; ++pre)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) af[pre][mt] = lda(pre, mt);
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        __builtin_amdgcn_sched_barrier(0);
        if (ks + kAhead < KSTEPS) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) af[(ks + kAhead) % (kAhead + 1)][mt] = lda(ks + kAhead, mt);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) s[mt] = mfma16<BF16>(af[ks % (kAhead + 1)][mt], qf[ks], s[mt]);
        under(ks);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// One online-softmax step; lane owns head c16 and keys mt*16 + 4g + r of the tile, masked keys arrive as -inf in s.  Scores stay unscaled:
// with cs = sm_scale * log2(e), P = exp2(S*cs - m) is one FMA + one v_exp_f32 per element; m_run / tmax are kept in the scaled log2 domain.
// Deferred rescale: the running reference m_run only moves when some head's tile maximum exceeds it by more than kDefer (then every head of
// the wave re-bases); otherwise P = exp2(.) <= 2^kDefer and neither l nor the 128 accumulators need touching.  out = acc / l is invariant to
// the reference.  Returns P^T in pf: k-step kk of P.V covers key tiles (2kk, 2kk+1); slots 0..3 / 4..7 of lane group g.
//
// WHOLE_REF = false: the reference re-bases to the true maximum; needs sm_scale > 0 and at least one unmasked key per tile.
// WHOLE_REF = true: the reference is kept a WHOLE number (m = ceil(max); the caller starts it from one, or from -inf).  P = exp2(x - m_run)
// then differs between two references by a power of two, which the rounding of P to the KV dtype commutes with -- the rounded P does not
// depend on the tile order, the split count or the value the reference starts from, and the partials of the pieces merge with exact weights.
// (Against the running maximum itself a row of three keys missed the tests' tolerance: each P's rounding error is relative to its term, the
// terms cancel.)  This form also serves a head whose keys of the tile are all masked and sm_scale = 0: -inf * 0 is kept out of tmax and of P.
template <bool BF16, bool WHOLE_REF>
__device__ __forceinline__ void softmax_step(const f32x4 (&s)[4], float cs, float &m_run, float &l_run, f32x4 (&acc)[32], s16x8 (&pf)[2])
{
    float tmax = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) tmax = fmaxf(fmaxf(tmax, fmaxf(s[mt][0], s[mt][1])), fmaxf(s[mt][2], s[mt][3]));
    tmax = max_over_rows(tmax);
    if constexpr (WHOLE_REF) tmax = tmax == -INFINITY ? tmax : tmax * cs;      // sm_scale >= 0: max commutes with the scaling
    else tmax *= cs;                                                         // sm_scale > 0
    constexpr float kDefer = 11.0f;                 // log2 domain (e^8 ~ 2^11.5)
    if (__any(tmax > m_run + kDefer)) {
        float m_new = fmaxf(m_run, tmax);
        if constexpr (WHOLE_REF) m_new = ceilf(m_new);
        const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);   // m_run = -inf -> 0
        l_run *= alpha;
        m_run = m_new;
#pragma unroll
        for (int c = 0; c < 4; ++c) {               // 8 accumulators at a time keeps the VGPR<->AGPR staging small
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[c * 8 + i] *= alpha;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float nm = (m_run == -INFINITY) ? 0.f : -m_run;
    float psum = 0.f;
    uint32_t pk[8];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[mt][r], cs, nm));
            if constexpr (WHOLE_REF) e[r] = s[mt][r] == -INFINITY ? 0.f : e[r];      // cs = 0: -inf * 0 is kept out
            psum += e[r];
        }
        pk[mt * 2 + 0] = pack2<BF16>(e[0], e[1]);
        pk[mt * 2 + 1] = pack2<BF16>(e[2], e[3]);
    }
    psum = sum_over_rows(psum);
    l_run += psum;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) pf[kk] = __builtin_bit_cast(s16x8, u32x4{pk[kk * 4 + 0], pk[kk * 4 + 1], pk[kk * 4 + 2], pk[kk * 4 + 3]});
}

// O^T[d, head] += V^T . P^T: V = the nope rows of the same LDS tile, transposed on the fly (two ds_read_b64_tr_b16 per MFMA); the
// sched_group_barrier sequence keeps kPvAhead MFMAs' worth of transpose reads in flight (<= 15 DS ops) and one MFMA per two reads after that.
template <bool BF16>
__device__ __forceinline__ void pv_accumulate(const uint8_t *buf, const s16x8 (&pf)[2], f32x4 (&acc)[32], int g, int c16)
{
    const uint8_t *vrow = buf + (4 * g + (c16 >> 2)) * kNopeStride + (c16 & 3) * 8;
    auto ldv = [&](int i, int half) -> s16x4 {      // i = kk * 32 + dt
        const int kk = i / 32, dt = i % 32;
        return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (s16x4 __attribute__((address_space(3))) *)(vrow + (2 * kk + half) * 16 * kNopeStride + dt * 32));
    };
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const s16x4 lo = ldv(i, 0), hi = ldv(i, 1);
        const s16x8 a = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[i % 32] = mfma16<BF16>(a, pf[i / 32], acc[i % 32]);
    }
    constexpr int kPvAhead = 8;
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * kPvAhead, 0);
#pragma unroll
    for (int i = 0; i < 64 - kPvAhead; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, kPvAhead, 0);
    __builtin_amdgcn_sched_barrier(0);
}

// The two finishes; lane holds O^T[d = dt*16 + 4g + r][head c16].  orow / po = the head's 512-element row.
template <bool BF16>
__device__ __forceinline__ void store_head_out(uint16_t *orow, const f32x4 (&acc)[32], float l_run, int g)
{
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    orow += 4 * g;
#pragma unroll
    for (int dt = 0; dt < 32; ++dt) {
        const uint32_t w0 = (uint32_t)cvt_out<BF16>(acc[dt][0] * inv) | ((uint32_t)cvt_out<BF16>(acc[dt][1] * inv) << 16);
        const uint32_t w1 = (uint32_t)cvt_out<BF16>(acc[dt][2] * inv) | ((uint32_t)cvt_out<BF16>(acc[dt][3] * inv) << 16);
        *(uint2 *)(orow + dt * 16) = uint2{w0, w1};
    }
}
// unnormalised fp32 partial of one piece plus its (m, l), for a merge kernel
__device__ __forceinline__ void store_head_partial(float *po, float *ml, const f32x4 (&acc)[32], float m_run, float l_run, int g)
{
    po += 4 * g;
#pragma unroll
    for (int dt = 0; dt < 32; ++dt) *(f32x4 *)(po + dt * 16) = acc[dt];
    if (g == 0) {
        ml[0] = m_run;
        ml[1] = l_run;
    }
}

}  // namespace mi_sgl
