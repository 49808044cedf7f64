"""Prefill block-score indexer (torch.ops.npu.gqa_prefill_block_score, "max") against what a user would write without it.

Per shape (bf16, D = 128): the score op over a varlen chunk, and the baseline -- per request `torch.matmul` of its rows [q_len * G, D]
with its gathered, contiguous K [D, seq_len] (the full rectangle, no causal mask, the gather itself not timed), then torch's per-block
`amax` of the result.  The baseline does about twice the useful work and answers a different question (its scores are not masked); it is
the time to beat, not a parity reference.  Both rotate over several disjoint page sets, alternate in one process, `rounds` windows each,
timed with device events after a warm-up.  Reported: median / min / max of the per-call time over the windows, the causal flops
(2 * D per visible (row, key) pair) over the median, and that rate as a fraction of the bf16 MFMA peak.  The select launch is timed too
(fused form, topk = 2048 / block keys), on its own.  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgl-kernel-npu_amd", "python"))
import torch

MFMA_PEAK = 2.5e15          # bf16 dense, FLOP/s
SHAPES = []
for G in (1, 4):
    for bs in (64, 128):
        for toks in (4096, 8192, 32768):
            SHAPES.append((f"g{G}_blk{bs}_1x{toks // 1024}k", G, bs, [(0, toks)]))
        SHAPES.append((f"g{G}_blk{bs}_8x1k_after_3k", G, bs, [(3072, 1024)] * 8))


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def bench_shape(name, G, bs, reqs, seed, rounds):
    import sgl_kernel_npu  # noqa: F401
    D, dtype = 128, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = len(reqs)
    lens = [a + b for a, b in reqs]
    total_q = sum(b for _, b in reqs)
    blocks = [-(-x // bs) for x in lens]
    kv_bytes = sum(lens) * D * 2
    sets = int(min(16, max(2, -(-(1 << 28) // kv_bytes))))
    pages_per_set = sum(blocks)
    k = torch.empty((sets * pages_per_set, bs, 1, D), dtype=dtype, device="cuda").normal_(generator=g)
    q = torch.randn((total_q, G, D), generator=g, device="cuda").to(dtype)
    cu = torch.tensor([0] + [b for _, b in reqs], device="cuda").cumsum(0).to(torch.int32)
    seq_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    pool = torch.arange(n, dtype=torch.int32, device="cuda")
    max_seqlen = max(lens)
    maps, dense = [], []
    for s in range(sets):
        perm = (torch.randperm(pages_per_set, generator=g, device="cuda") + s * pages_per_set).tolist()
        rtt = torch.zeros((n, max(blocks) * bs), dtype=torch.int32, device="cuda")
        per_req = []
        for r in range(n):
            pg = torch.tensor([perm.pop() for _ in range(blocks[r])], device="cuda")
            rtt[r, :blocks[r] * bs] = (pg[:, None] * bs + torch.arange(bs, device="cuda")[None, :]).reshape(-1).to(torch.int32)
            per_req.append(k[pg, :, 0].reshape(-1, D).t().contiguous())      # the baseline's gathered K [D, blocks * bs]
        maps.append(rtt)
        dense.append(per_req)
    sm = D ** -0.5
    topk = max(1, 2048 // bs)
    pos = torch.cat([torch.arange(a, a + b) for a, b in reqs])
    pq = (pos + 1).to(torch.int32).cuda()
    starts = [sum(b for _, b in reqs[:r]) for r in range(n + 1)]

    def run_score(i):
        return torch.ops.npu.gqa_prefill_block_score(q, k, cu, seq_lens, maps[i % sets], pool, max_seqlen, sm, False, None)

    def run_baseline(i):
        out = []
        for r, (a, b) in enumerate(reqs):
            rows = q[starts[r]:starts[r + 1]].reshape(-1, D)
            s = torch.matmul(rows, dense[i % sets][r])
            out.append(s.view(s.shape[0], blocks[r], bs).amax(dim=2))
        return out

    score = run_score(0)

    def run_select(i):
        return torch.ops.npu.prefill_topk_from_score(score[:1], pq, topk, bs, True)

    torch.cuda.synchronize()
    fns = dict(score=run_score, baseline=run_baseline, select=run_select)
    calls = {}
    for label, fn in fns.items():
        for i in range(max(3, sets)):
            fn(i)
        torch.cuda.synchronize()
        t = window(fn, 3)
        calls[label] = int(min(2000, max(3, 50e3 / t)))                 # windows of about 50 ms
    times = {label: [] for label in fns}
    for _ in range(rounds):
        for label, fn in fns.items():
            times[label].append(window(fn, calls[label]))
    pairs = int((pos + 1).sum()) * G
    flops = 2 * D * pairs
    res = dict(shape=dict(G=G, kv_heads=1, D=D, block_size=bs, requests=reqs, total_q=total_q, dtype="bfloat16", score_type="max", select_topk=topk),
               page_sets_rotated=sets, causal_flops=flops, baseline_flops=2 * D * G * sum(b * bl * bs for (_, b), bl in zip(reqs, blocks)))
    for label, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[label] = dict(median_us=med, min_us=ts[0], max_us=ts[-1], calls_per_window=calls[label], windows=rounds)
        if label != "select":
            res[label].update(causal_flops_per_s=flops / (med * 1e-6), share_of_bf16_mfma_peak=flops / (med * 1e-6) / MFMA_PEAK)
    res["score_time_over_baseline"] = res["score"]["median_us"] / res["baseline"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, help="one shape name")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
    torch.cuda.set_device(0)
    out = dict(device=torch.cuda.get_device_name(0), bf16_mfma_peak_flop_per_s=MFMA_PEAK, timing="device events, per-call time of a window",
               tool="tools/bench_block_score_prefill.py", shapes={})
    for name, *shape in SHAPES:
        if a.only and a.only != name:
            continue
        out["shapes"][name] = bench_shape(name, *shape, a.seed, a.rounds)
        torch.cuda.empty_cache()
        if a.out:                                               # kept up to date shape by shape
            with open(a.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
