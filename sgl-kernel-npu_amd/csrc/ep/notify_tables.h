// The notify exchange's count tables (see mi_ep.h), derived by one workgroup from the W x (E + 1) count matrix.  Shared by the
// notify kernels (sync.hip) and the one-launch single-rank dispatch (dispatch.hip, stage_local_kernel<..., TABLES = true>).
#pragma once
#include "ep_common.h"

namespace mi_ep {

// One workgroup; L*W <= 2048 entries.  See mi_ep.h for the table definitions
// (reference notify_dispatch.h:386-407,434-450,473-482,553-577,606-615,665-669,715-721,759-780).
// Everything the serial reference core loops over is staged in LDS first (one coalesced pass over the counts), the
// per-source sender prefixes are wave reductions, the short dependent scans run out of LDS: ~3 us instead of ~28 us.
__device__ __forceinline__ int32_t wave_incl_scan(int32_t v, int) { return wave_incl_scan_i32(v); }

__device__ void notify_tables_body(
    const int32_t *__restrict__ cnt /*[W][E+1]*/, int W, int E, int me, int relative_pull,
    int32_t *__restrict__ recv_count, int32_t *__restrict__ recv_offset, int32_t *__restrict__ recv_tokens_per_expert,
    int32_t *__restrict__ expert_global_offset, int32_t *__restrict__ srcrank_in_expert_offset,
    int32_t *__restrict__ r_in_srcrank_offset, int32_t *__restrict__ total_recv_token, int32_t *__restrict__ max_bs,
    int32_t *__restrict__ pull_offset, int32_t *summary_host, int32_t *sm)
{
    const int L = E / W;
    const int LW = L * W;
    int32_t *c = sm;                 // [L*W] counts in idx-i order
    int32_t *pre = sm + LW;          // [W] sender prefix at my first expert
    int32_t *ego = pre + W;          // [L+1]
    int32_t *sie = ego + L + 1;      // [L*W] exclusive scan over src inside one local expert
    int32_t *mbs = sie + LW;         // [1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    // counts of my experts, idx-i order (coalesced over le for a fixed src)
    for (int i = tid; i < LW; i += blockDim.x) {
        const int le = i / W, src = i % W;
        c[i] = cnt[(size_t)src * (E + 1) + me * L + le];
    }
    // sender-side exclusive prefix up to my first expert: one wave per source rank
    for (int src = wave; src < W; src += nwaves) {
        const int32_t *row = cnt + (size_t)src * (E + 1);
        int32_t s = 0;
        for (int e = lane; e < me * L; e += 64) s += row[e];
        s = wave_sum_i32(s);
        if (lane == 0) pre[src] = s;
    }
    if (wave == 0) {
        int32_t mb = 0;
        for (int src = lane; src < W; src += 64) mb = max(mb, cnt[(size_t)src * (E + 1) + E]);
        mb = wave_max_i32(mb);
        if (lane == 0) mbs[0] = mb;
    }
    __syncthreads();
    // per source: running sender offset over my experts -- one wave per source, 64 experts per step
    for (int src = wave; src < W; src += nwaves) {
        int32_t carry = pre[src];
        for (int le0 = 0; le0 < L; le0 += 64) {
            const int le = le0 + lane;
            const int32_t v = le < L ? c[le * W + src] : 0;
            const int32_t inc = wave_incl_scan(v, lane);
            if (le < L) {
                const int32_t run = carry + inc - v;
                recv_offset[le * W + src] = run;
                pull_offset[le * W + src] = relative_pull ? run - pre[src] : run;
            }
            carry += __builtin_amdgcn_readlane(inc, 63);
        }
    }
    // per local expert: scan over sources (W <= 64 values: serial per thread, experts in parallel)
    for (int le = tid; le < L; le += blockDim.x) {
        int32_t s = 0;
        for (int src = 0; src < W; ++src) {
            sie[le * W + src] = s;
            s += c[le * W + src];
        }
        ego[le] = s;
        recv_tokens_per_expert[le] = s;
    }
    __syncthreads();
    if (wave == 0) {                 // exclusive scan of the per-expert totals, 64 per step
        int32_t carry = 0;
        for (int le0 = 0; le0 < L; le0 += 64) {
            const int le = le0 + lane;
            const int32_t v = le < L ? ego[le] : 0;
            const int32_t inc = wave_incl_scan(v, lane);
            if (le < L) ego[le] = carry + inc - v;
            carry += __builtin_amdgcn_readlane(inc, 63);
        }
        if (lane == 0) ego[L] = carry;
    }
    __syncthreads();
    if (summary_host) {
        // The host's words go out first (they cross PCIe while the tables below are stored), every word exactly once, >= 0, in NO
        // particular order and with no fence: the host pre-sets every word it reads to -1 and waits for each.  (Per-expert counts, a
        // barrier, a system fence and a release store of the total -- the ordered form -- kept the workgroup waiting for two PCIe
        // write round trips: ~3 us of the 4.8 us this phase took.)
        for (int le = tid; le < L; le += blockDim.x)
            __hip_atomic_store(summary_host + 2 + le, ego[le + 1] - ego[le], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (tid == 0) {
            __hip_atomic_store(summary_host + 1, mbs[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(summary_host + 0, ego[L], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    for (int i = tid; i < LW; i += blockDim.x) {
        const int le = i / W;
        srcrank_in_expert_offset[i] = sie[i];
        r_in_srcrank_offset[i] = 0;
        recv_count[i] = ego[le] + sie[i] + c[i];
    }
    for (int le = tid; le < L; le += blockDim.x) expert_global_offset[le] = ego[le];
    if (tid == 0) {
        total_recv_token[0] = ego[L];
        max_bs[0] = mbs[0];
    }
}

}  // namespace mi_ep
