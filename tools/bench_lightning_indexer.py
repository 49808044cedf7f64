"""Lightning indexer (torch.ops.npu.lightning_indexer) against the block-score indexer (flash_decode_bnsd_with_topk_idx, score-only form,
64 query heads / 1 kv head, D = 128, blocks of 128 keys) at the same batch and context: both read every K byte of the context once per
step, with the same MFMA work per byte.

bf16, sparse_count 2048, block_size 128, causal.  Decode: S1 = 1 (TND), B in {1, 32, 128}, context in {8 k, 64 k}; MTP: S1 = 2 (BSND) at
the same batches and contexts; prefill: one TND sequence of 4096 tokens over its own 4096 keys (no comparator: the block-score decode
kernel has no such form).  Every sequence is 37 keys short of the context, so the last page is partly filled.  Per shape the variants run
over the same block tables, rotate over several disjoint page sets (about 1 GiB of K) so that consecutive calls do not find their keys in
the last-level cache, and alternate in one process, `rounds` windows each, timed with device events after a warm-up.

Reported per shape: us per call of the op (score + select launches), of the score launch alone (mi_lightning_indexer_score through the
C-ABI) and, as their difference, of the select launch; the K bytes (sum_b len_b x 256 B) per second of the score launch and of the op; the
comparator's us per call and K bytes per second; and score_rate_over_block_score, the figure to watch: the aim is >= 1.

Without --only the tool is a driver: every shape runs in a child process of its own under `timeout`, and the first shape that fails ends
the run (nothing more is started on the GPU).  One JSON object on stdout (and in --out)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgl-kernel-npu_amd", "python"))
import torch

HBM_PEAK = 8.0e12
BS, COUNT, HEADS, D = 128, 2048, 64, 128
SHAPES = ([(f"decode_b{B}_{ctx // 1024}k", "decode", B, 1, ctx) for B in (1, 32, 128) for ctx in (8192, 65536)]
          + [(f"mtp_b{B}_{ctx // 1024}k", "mtp", B, 2, ctx) for B in (1, 32, 128) for ctx in (8192, 65536)]
          + [("prefill_t4096_4k", "prefill", 1, 4096, 4096 + 37)])
CHILD_TIMEOUT_S = 170


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def score_entry():
    lib = ctypes.CDLL(os.path.join(ROOT, "sgl-kernel-npu_amd", "lib", "libmi_sgl_kernels.so"))
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.mi_lightning_indexer_score.argtypes = [P] * 4 + [L] + [P] * 3 + [I, I, I, I, L, I, I, I, L, I] + [L] * 8 + [I, I, P]
    return lib.mi_lightning_indexer_score


def bench_shape(name, kind, B, S1, ctx, seed, rounds):
    import sgl_kernel_npu  # noqa: F401
    from sgl_kernel_npu.indexer.flash_block_score_decode import flash_decode_bnsd_with_topk_idx as block_indexer
    dtype = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(seed)
    blocks = -(-ctx // BS)
    k_bytes = B * blocks * BS * D * 2
    sets = int(min(16, max(2, -(-(1 << 30) // k_bytes))))             # rotate over about 1 GiB of K, at least two sets
    num_pages = sets * B * blocks
    k = torch.empty((num_pages, BS, 1, D), dtype=dtype, device="cuda").normal_(generator=g)
    tables = torch.randperm(num_pages, generator=g, device="cuda").to(torch.int32).reshape(sets, B, blocks)
    lens = torch.full((B,), ctx - 37, dtype=torch.int32, device="cuda")
    tnd = kind != "mtp"
    rows = B * S1
    q = torch.randn((rows, HEADS, D) if tnd else (B, S1, HEADS, D), generator=g, device="cuda").to(dtype)
    w = torch.randn((rows, HEADS) if tnd else (B, S1, HEADS), generator=g, device="cuda").to(dtype)
    cu = (torch.arange(1, B + 1, dtype=torch.int32, device="cuda") * S1) if tnd else None
    layout = "TND" if tnd else "BSND"
    cap = blocks * BS
    ld = -(-cap // 64) * 64
    scores = torch.empty((rows, ld), dtype=torch.float32, device="cuda")
    score_fn = score_entry()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())

    def run_op(i):
        return torch.ops.npu.lightning_indexer(q, k, w, actual_seq_lengths_query=cu, actual_seq_lengths_key=lens, block_table=tables[i % sets],
                                               layout_query=layout, layout_key="PA_BSND", sparse_count=COUNT, sparse_mode=3)

    def run_score(i):
        t = tables[i % sets]
        rc = score_fn(ptr(q), ptr(k), ptr(w), ptr(scores), ld, ptr(cu), ptr(lens), ptr(t), 1 if tnd else 0, 2, B, 1 if tnd else S1, rows, HEADS, 1,
                      D, cap, BS, t.stride(0), q.stride(0), 0 if tnd else q.stride(1), q.stride(-2), w.stride(0), 0 if tnd else w.stride(1),
                      k.stride(0), k.stride(1), 3, 0, stream)
        assert rc == 0, rc

    variants = {"op": run_op, "score": run_score}
    if kind != "prefill":
        qb = torch.randn((B, HEADS, D), generator=g, device="cuda").to(dtype)
        topk = COUNT // BS

        def run_block(i):
            return block_indexer(qb, None, k, None, tables[i % sets], lens, ctx, BS, topk, 0, 0, D ** -0.5, "max", disable_index_value=True)[1]

        variants["block_score"] = run_block
    idx = run_op(0)
    torch.cuda.synchronize()
    assert int(idx.max()) < ctx - 37 and int(idx.min()) >= -1
    for fn in variants.values():
        for i in range(3 * sets):
            fn(i)
    torch.cuda.synchronize()
    calls = {label: int(min(2000, max(5, 50e3 / window(fn, 5)))) for label, fn in variants.items()}      # windows of about 50 ms
    times = {label: [] for label in variants}
    for _ in range(rounds):
        for label, fn in variants.items():
            times[label].append(window(fn, calls[label]))
    keys = int(lens.sum())
    nbytes = keys * D * 2                                                # K leaves HBM once per sequence
    res = dict(shape=dict(kind=kind, B=B, S1=S1, context=ctx, layout_query=layout, block_size=BS, sparse_count=COUNT, sparse_mode=3, dtype="bfloat16"),
               page_sets_rotated=sets, rotation_working_set_bytes=k_bytes * sets, k_bytes=nbytes)
    for label, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[label] = dict(median_us=med, min_us=ts[0], max_us=ts[-1], calls_per_window=calls[label], windows=rounds,
                          k_bytes_per_s=nbytes / (med * 1e-6), share_of_hbm_peak=nbytes / (med * 1e-6) / HBM_PEAK)
    res["select_us_by_difference"] = res["op"]["median_us"] - res["score"]["median_us"]
    if kind == "prefill":
        visible = sum(min(max(ctx - 37 - (S1 - 1 - r), 0), ctx - 37) for r in range(S1))
        res["score"]["mfma_flops_per_s"] = 2.0 * S1 * (ctx - 37) * HEADS * D / (res["score"]["median_us"] * 1e-6)
        res["visible_scores"] = visible
    else:
        res["score_rate_over_block_score"] = res["score"]["k_bytes_per_s"] / res["block_score"]["k_bytes_per_s"]
        res["aim_met"] = res["score_rate_over_block_score"] >= 1.0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, help="one shape name, measured in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    by_name = {s[0]: s for s in SHAPES}
    if a.only:
        assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
        torch.cuda.set_device(0)
        out = dict(device=torch.cuda.get_device_name(0), result=bench_shape(*by_name[a.only], a.seed, a.rounds))
    else:
        out = dict(hbm_peak_bytes_per_s=HBM_PEAK, timing="device events, per-call time of a window", tool="tools/bench_lightning_indexer.py",
                   comparator="flash_decode_bnsd_with_topk_idx, score-only, 64 q heads / 1 kv head, D 128, blocks of 128, measured in the same run",
                   shapes={})
        with tempfile.TemporaryDirectory() as tmp:
            for name in by_name:
                path = os.path.join(tmp, name + ".json")
                cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--only", name, "--seed",
                       str(a.seed), "--rounds", str(a.rounds), "--out", path]
                rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
                if rc != 0:
                    out["stopped"] = f"shape {name} ended with status {rc}: nothing more was started"
                    break
                with open(path) as f:
                    child = json.load(f)
                out["device"] = child["device"]
                out["shapes"][name] = child["result"]
                print(name, json.dumps(child["result"].get("score_rate_over_block_score")), file=sys.stderr, flush=True)
        rates = [s["score_rate_over_block_score"] for s in out["shapes"].values() if "score_rate_over_block_score" in s]
        if rates:
            out["score_rate_over_block_score_min"], out["score_rate_over_block_score_max"] = min(rates), max(rates)
            out["aim_met_on_every_shape"] = all(r >= 1.0 for r in rates)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    if "stopped" in out:
        sys.exit(1)


if __name__ == "__main__":
    main()
