"""Block-score indexer (flash_decode_bnsd_with_topk_idx, score-only form) against the dense paged decode (decode_gqa) at the same shapes.

The indexer reads every K byte of the context once per step; decode_gqa reads K and V.  Per shape both run over the same block tables and
lengths (every sequence 37 keys short of the context, so the last block is partly filled), rotate over several disjoint page sets so that
consecutive calls do not find their keys in the last-level cache, and alternate in one process, `rounds` windows each, timed with device
events after a warm-up.  Reported per variant: median / min / max of the per-call time over the windows, the algorithmic bytes
(sum_b len_b x Hkv x D x 2 B of K, plus q, for the indexer; K and V, plus q and out, for decode_gqa) and bytes/s; per shape the indexer's
bytes/s as a fraction of decode_gqa's -- the figure to watch: the indexer has no V, no P.V and no accumulator, so it should move its bytes
at least as fast.  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgl-kernel-npu_amd", "python"))
import torch

HBM_PEAK = 8.0e12
SHAPES = [(f"b{B}_h64_kv8_d128_blk{bs}_{ctx // 1024}k", B, 64, 8, 128, bs, ctx) for B in (1, 32, 128) for bs in (128, 16) for ctx in (4096, 32768)]


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def bench_shape(name, B, Hq, Hkv, D, bs, ctx, dtype, seed, rounds, score_type):
    from sgl_kernel_npu.attention.decode_attention import decode_gqa
    from sgl_kernel_npu.indexer.flash_block_score_decode import flash_decode_bnsd_with_topk_idx as indexer
    g = torch.Generator(device="cuda").manual_seed(seed)
    blocks = ctx // bs
    kv_bytes = B * ctx * Hkv * D * 2
    sets = int(min(16, max(2, -(-(1 << 30) // kv_bytes))))             # rotate over about 1 GiB of K, at least two sets
    num_pages = sets * B * blocks
    k = torch.empty((num_pages, bs, Hkv, D), dtype=dtype, device="cuda").normal_(generator=g)
    v = torch.empty((num_pages, bs, Hkv, D), dtype=dtype, device="cuda").normal_(generator=g)
    q = torch.randn((B, Hq, D), generator=g, device="cuda").to(dtype)
    tables = torch.randperm(num_pages, generator=g, device="cuda").to(torch.int32).reshape(sets, B, blocks)
    lens = torch.full((B,), ctx - 37, dtype=torch.int32, device="cuda")
    topk = max(1, 2048 // bs)
    dense_out = torch.empty_like(q)
    sm = D ** -0.5

    def run_score(i):
        return indexer(q, None, k, None, tables[i % sets], lens, ctx, bs, topk, 0, 0, sm, score_type, disable_index_value=True)[1]

    def run_dense(i):
        decode_gqa(q, k, v, dense_out, lens, sm, bs, tables[i % sets])

    idx = run_score(0)
    torch.cuda.synchronize()
    assert idx.shape == (Hq, B, topk) and int(idx.min()) >= 0 and int(idx.max()) < blocks
    for fn in (run_score, run_dense):
        for i in range(3 * sets):
            fn(i)
    torch.cuda.synchronize()
    calls = {}
    for label, fn in (("score", run_score), ("dense", run_dense)):
        t = window(fn, 20)
        calls[label] = int(min(2000, max(20, 50e3 / t)))               # windows of about 50 ms
    times = {"score": [], "dense": []}
    for _ in range(rounds):
        times["score"].append(window(run_score, calls["score"]))
        times["dense"].append(window(run_dense, calls["dense"]))
    keys = int(lens.sum())
    nbytes = {"score": keys * Hkv * D * 2 + B * Hq * D * 2, "dense": 2 * keys * Hkv * D * 2 + 2 * B * Hq * D * 2}
    res = dict(shape=dict(B=B, Hq=Hq, Hkv=Hkv, D=D, block_size=bs, context=ctx, topk=topk, score_type=score_type, dtype=str(dtype).split(".")[-1]),
               page_sets_rotated=sets, rotation_working_set_bytes=kv_bytes * sets)
    for label, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[label] = dict(median_us=med, min_us=ts[0], max_us=ts[-1], calls_per_window=calls[label], windows=rounds, algorithmic_bytes=nbytes[label],
                          bytes_per_s=nbytes[label] / (med * 1e-6), share_of_hbm_peak=nbytes[label] / (med * 1e-6) / HBM_PEAK)
    res["score_bytes_per_s_over_dense"] = res["score"]["bytes_per_s"] / res["dense"]["bytes_per_s"]
    res["score_time_over_dense"] = res["score"]["median_us"] / res["dense"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    ap.add_argument("--score-type", default="max", choices=["max", "lse"])
    ap.add_argument("--only", default=None, help="one shape name")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
    torch.cuda.set_device(0)
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, timing="device events, per-call time of a window",
               tool="tools/bench_block_score.py", shapes={})
    for name, *shape in SHAPES:
        if a.only and a.only != name:
            continue
        out["shapes"][name] = bench_shape(name, *shape, getattr(torch, a.dtype), a.seed, a.rounds, a.score_type)
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
