"""Block-sparse GQA decode (flash_decode_bnsd_with_gqa_share_sparse) against the dense paged decode (decode_gqa) over the same keys.

Per shape: every sequence selects topk - 1 random full blocks of its context plus its last, partly filled block (last in the list); the
comparator runs decode_gqa on a block table that names exactly the pages of kv head 0's list, i.e. a dense sequence of the same number of
attended keys that reads the same bytes.  Both rotate over several independent selections so that consecutive calls do not find their keys
in the last-level cache; they alternate in one process, `rounds` windows each, timed with device events after a warm-up.  Reported per
variant: median / min / max of the per-call time over the windows, the algorithmic bytes (attended keys x D x 2 B x 2 for K and V per kv
head, plus q and out) and bytes/s as a share of the 8 TB/s HBM peak.  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgl-kernel-npu_amd", "python"))
import torch

HBM_PEAK = 8.0e12
SHAPES = [  # name, B, Hq, Hkv, D, block, topk, context
    ("b4_h16_kv1_blk128_top17_32k", 4, 16, 1, 128, 128, 17, 32768),
    ("b128_h16_kv1_blk128_top17_32k", 128, 16, 1, 128, 128, 17, 32768),
    ("b64_h64_kv8_blk64_top32_16k", 64, 64, 8, 128, 64, 32, 16384),
]


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def bench_shape(name, B, Hq, Hkv, D, bs, topk, ctx, dtype, seed, sets, rounds):
    from sgl_kernel_npu.attention.decode_attention import decode_gqa
    from sgl_kernel_npu.attention.gqa_share_sparse_attention import flash_decode_bnsd_with_gqa_share_sparse as sparse
    g = torch.Generator(device="cuda").manual_seed(seed)
    blocks = ctx // bs
    num_pages = B * blocks
    k = torch.empty((num_pages, bs, Hkv, D), dtype=dtype, device="cuda").normal_(generator=g)
    v = torch.empty((num_pages, bs, Hkv, D), dtype=dtype, device="cuda").normal_(generator=g)
    q = torch.randn((B, Hq, D), generator=g, device="cuda").to(dtype)
    bt = torch.randperm(num_pages, generator=g, device="cuda").to(torch.int32).reshape(B, blocks)
    tail = bs - 37                                                     # keys in the last block of every sequence
    lens = torch.full((B,), ctx - 37, dtype=torch.int32, device="cuda")
    lists, dense_bt = [], []
    for _ in range(sets):
        scores = torch.rand((Hkv, B, blocks - 1), generator=g, device="cuda")
        sel = torch.topk(scores, topk - 1, dim=-1)[1].to(torch.int32)
        idx = torch.cat([sel, torch.full((Hkv, B, 1), blocks - 1, dtype=torch.int32, device="cuda")], dim=-1).contiguous()
        lists.append(idx)
        dense_bt.append(torch.gather(bt, 1, idx[0].long()).contiguous())      # the pages of kv head 0's list, the partly filled one last
    keys = (topk - 1) * bs + tail
    dense_lens = torch.full((B,), keys, dtype=torch.int32, device="cuda")
    dense_out = torch.empty_like(q)
    sm = D ** -0.5
    chunks = int(torch.ops.npu.gqa_share_sparse_num_chunks(B, Hkv, topk))
    chunks = min(chunks, 8)                                            # what the Python entry point picks with its default bound

    def run_sparse(i):
        return sparse(q, None, k, v, bt, lens, bs, lists[i % sets], sm)

    def run_dense(i):
        decode_gqa(q, k, v, dense_out, dense_lens, sm, bs, dense_bt[i % sets])

    # same keys -> same result (kv head 0's heads; all heads when there is one kv head)
    got = run_sparse(0)
    run_dense(0)
    torch.cuda.synchronize()
    G = Hq // Hkv
    diff = (got[:, :G].float() - dense_out[:, :G].float()).abs().max().item()
    for fn in (run_sparse, run_dense):
        for i in range(3 * sets):
            fn(i)
    torch.cuda.synchronize()
    calls = {}
    for label, fn in (("sparse", run_sparse), ("dense", run_dense)):
        t = window(fn, 20)
        calls[label] = int(min(2000, max(20, 50e3 / t)))               # windows of about 50 ms
    times = {"sparse": [], "dense": []}
    for _ in range(rounds):
        times["sparse"].append(window(run_sparse, calls["sparse"]))
        times["dense"].append(window(run_dense, calls["dense"]))
    nbytes = B * Hkv * keys * D * 2 * 2 + 2 * B * Hq * D * 2
    res = dict(shape=dict(B=B, Hq=Hq, Hkv=Hkv, D=D, block_size=bs, topk=topk, context=ctx, dtype=str(dtype).split(".")[-1]),
               attended_keys_per_kv_head=keys, algorithmic_bytes=nbytes, num_topk_chunks=chunks, selections_rotated=sets,
               rotation_working_set_bytes=nbytes * sets, max_abs_diff_sparse_vs_dense=diff)
    for label, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[label] = dict(median_us=med, min_us=ts[0], max_us=ts[-1], calls_per_window=calls[label], windows=rounds,
                          bytes_per_s=nbytes / (med * 1e-6), share_of_hbm_peak=nbytes / (med * 1e-6) / HBM_PEAK)
    res["sparse_over_dense"] = res["sparse"]["median_us"] / res["dense"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    ap.add_argument("--only", default=None, help="one shape name")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
    torch.cuda.set_device(0)
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, timing="device events, per-call time of a window",
               shapes={})
    for name, *shape in SHAPES:
        if a.only and a.only != name:
            continue
        out["shapes"][name] = bench_shape(name, *shape, getattr(torch, a.dtype), a.seed, a.sets, a.rounds)
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
