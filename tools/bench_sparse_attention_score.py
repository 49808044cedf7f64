"""torch.ops.npu.npu_sparse_attention_score at the MiniMax-M3 shape (Hq 8, Hkv 1, D 128, block 128, topK 17) with 16k keys per request:
decode (one token per request) at batch 1 / 16 / 128 and verify (4 tokens per request), in bf16, fp16 and FP8 (e4m3fn q / k / v with
per-block scales, fp16 out).

The yardstick is the existing block-sparse decode kernel (torch.ops.npu.gqa_share_sparse_decode -> mi_gqa_sparse_decode, the library's
chunk count) at the identical decode shape, on the same caches, tables and lists, timed in the same process in alternating windows; its
spread (min .. max of the per-call time over the windows, as a share of the median) is recorded beside it, and a decode row of the new op
counts as equal when its median lies inside the baseline's min .. max.  Decode rows are timed twice: with actual_seq_lengths = ones (every
wave scans the length vectors) and with actual_seq_lengths = None (one token per request: the scalar path).

Every token selects topK - 1 random full blocks of its context plus its diagonal block (last in the list).  The caches are a pool of 16384
pages (1 GiB of bf16 K + V); calls rotate over `sets` independent (table, list) selections drawn from the whole pool, enough of them that one
rotation moves at least 512 MB, so consecutive calls do not find their keys in the last-level cache.  Timed with device events around
windows of about 50 ms after a warm-up of every selection.  Per row: median / min / max of the per-call time over the windows, the selected
bytes (contributing keys x D x element size x 2 for K and V, plus q and out) and bytes/s as a share of the 8 TB/s HBM peak.  One JSON object
on stdout (and in --out)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgl-kernel-npu_amd", "python"))
import torch

HBM_PEAK = 8.0e12
HQ, HKV, D, BS, TOPK, CTX = 8, 1, 128, 128, 17, 16384
POOL_PAGES = 16384
ROWS = [  # name, batch, query tokens per request
    ("decode_b1", 1, 1), ("decode_b16", 16, 1), ("decode_b128", 128, 1), ("verify4_b1", 1, 4), ("verify4_b16", 16, 4), ("verify4_b128", 128, 4),
]
DTYPES = ["bfloat16", "float16", "float8_e4m3fn"]


_capi = None


def capi():
    """The C-ABI library, for the chunk count the op picks (host arithmetic)."""
    global _capi
    if _capi is None:
        _capi = ctypes.CDLL(os.path.join(ROOT, "sgl-kernel-npu_amd", "lib", "libmi_sgl_kernels.so"))
        _capi.mi_sparse_attention_score_num_chunks.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    return _capi


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def stats(ts, nbytes, calls):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return dict(median_us=med, min_us=ts[0], max_us=ts[-1], spread_of_median=(ts[-1] - ts[0]) / med, calls_per_window=calls, windows=len(ts),
                bytes_per_s=nbytes / (med * 1e-6), share_of_hbm_peak=nbytes / (med * 1e-6) / HBM_PEAK)


def bench_row(pool, B, qn, dtype, seed, rounds):
    """pool: dict dtype-name -> (k, v) caches of POOL_PAGES pages."""
    import sgl_kernel_npu  # noqa: F401
    op, old = torch.ops.npu.npu_sparse_attention_score, torch.ops.npu.gqa_share_sparse_decode
    g = torch.Generator(device="cuda").manual_seed(seed)
    fp8 = dtype == torch.float8_e4m3fn
    k, v = pool[dtype]
    esize = 1 if fp8 else 2
    blocks = CTX // BS
    T = B * qn
    kv_len = CTX - 37                                                  # the last token stands at position kv_len - 1, inside the last block
    pos = torch.arange(kv_len - qn, kv_len, device="cuda").repeat(B)   # [T]
    diag = (pos // BS).to(torch.int32)
    keys = int(((TOPK - 1) * BS + pos % BS + 1).sum().item())          # contributing keys over all tokens (one kv head)
    nbytes = keys * D * esize * 2 + T * HQ * D * (esize + 2)
    sets = int(min(512, max(8, -(-512e6 // nbytes))))
    q = torch.randn((T, HQ, D), generator=g, device="cuda").to(dtype)
    q_lens = torch.full((B,), qn, dtype=torch.int32, device="cuda")
    kv_lens = torch.full((B,), kv_len, dtype=torch.int32, device="cuda")
    tables, lists = [], []
    for _ in range(sets):
        tables.append(torch.randperm(POOL_PAGES, generator=g, device="cuda")[:B * blocks].to(torch.int32).reshape(B, blocks).contiguous())
        scores = torch.rand((HKV, T, blocks - 1), generator=g, device="cuda")      # the diagonal block is the last one for every token
        sel = torch.topk(scores, TOPK - 1, dim=-1)[1].to(torch.int32)
        lists.append(torch.cat([sel, diag.view(1, T, 1)], dim=-1).contiguous())
    kw = dict(actual_seq_lengths=q_lens, actual_seq_lengths_kv=kv_lens, num_key_value_heads=HKV, scale_value=D ** -0.5, block_size=BS, top_k=TOPK,
              inner_precise=4)
    if fp8:
        kw.update(q_dequant_scale=torch.rand((B, HQ, blocks), generator=g, device="cuda") * 0.01 + 0.005,
                  k_dequant_scale=torch.rand((B, HKV, blocks), generator=g, device="cuda") * 0.01 + 0.005,
                  v_dequant_scale=torch.rand((B, HKV, blocks), generator=g, device="cuda") * 0.01 + 0.005)

    def run_new(i):
        return op(q, k, v, lists[i % sets], tables[i % sets], **kw)

    kw_none = dict(kw, actual_seq_lengths=None)                        # one token per request without the length vector: the scalar path

    def run_new_none(i):
        return op(q, k, v, lists[i % sets], tables[i % sets], **kw_none)

    def run_old(i):
        return old(q, None, k, v, tables[i % sets], kv_lens, lists[i % sets], D ** -0.5, 0)

    runs = {"sparse_attention_score": run_new}
    res = dict(shape=dict(batch=B, tokens_per_request=qn, Hq=HQ, Hkv=HKV, D=D, block_size=BS, topk=TOPK, context=CTX, dtype=str(dtype).split(".")[-1]),
               contributing_keys=keys, selected_bytes=nbytes, selections_rotated=sets, rotation_working_set_bytes=nbytes * sets,
               num_chunks=int(capi().mi_sparse_attention_score_num_chunks(T, HKV, TOPK)))
    if qn == 1:
        runs["sparse_attention_score_no_actual_seq_lengths"] = run_new_none
    if qn == 1 and not fp8:                                            # the identical decode shape: the existing kernel on the same inputs
        runs["gqa_sparse_decode_baseline"] = run_old
        res["max_abs_diff_vs_baseline"] = (run_new(0).float() - run_old(0).float()).abs().max().item()
    for fn in runs.values():
        for i in range(sets + 8):
            fn(i)
    torch.cuda.synchronize()
    calls = {}
    for label, fn in runs.items():
        t = window(fn, 20)
        calls[label] = int(min(4000, max(20, 50e3 / t)))               # windows of about 50 ms
    times = {label: [] for label in runs}
    for _ in range(rounds):                                            # alternating windows
        for label, fn in runs.items():
            times[label].append(window(fn, calls[label]))
    for label, ts in times.items():
        res[label] = stats(ts, nbytes, calls[label])
    if "gqa_sparse_decode_baseline" in res:
        new, base = res["sparse_attention_score"], res["gqa_sparse_decode_baseline"]
        res["new_over_baseline"] = new["median_us"] / base["median_us"]
        res["within_baseline_spread"] = base["min_us"] <= new["median_us"] <= base["max_us"]
        none = res["sparse_attention_score_no_actual_seq_lengths"]
        res["no_actual_seq_lengths_over_baseline"] = none["median_us"] / base["median_us"]
        res["no_actual_seq_lengths_within_baseline_spread"] = base["min_us"] <= none["median_us"] <= base["max_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--only", default=None, help="one row name")
    ap.add_argument("--dtypes", default=",".join(DTYPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_attention_score_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    pool = {}
    for name in a.dtypes.split(","):
        dtype = getattr(torch, name)
        make = lambda: torch.empty((POOL_PAGES, BS, HKV, D), dtype=torch.bfloat16, device="cuda").normal_(generator=g)
        if dtype == torch.float8_e4m3fn:                               # values as the quantised caches hold them: spread over the format's range
            pool[dtype] = tuple((make() * 100).to(dtype) for _ in range(2))
        else:
            pool[dtype] = tuple(make().to(dtype) for _ in range(2))
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, timing="device events, per-call time of a window", rows={})
    for name, B, qn in ROWS:
        if a.only and a.only != name:
            continue
        for dtype in pool:
            out["rows"][f"{name}_{str(dtype).split('.')[-1]}"] = bench_row(pool, B, qn, dtype, a.seed, a.rounds)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
