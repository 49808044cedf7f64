"""sparse_attn_sharedkv (torch.ops.npu.sparse_attn_sharedkv) against decode_mla with 64 heads over a CONTIGUOUS sequence of the same number
of keys: the gather should move its bytes at no less than the contiguous read's rate.

bf16, decode (S1 = 1, BSND), B in {1, 32, 128}, pages of 128.  Sparse: window 128 + K in {512, 1024} index slots at cmp_ratio 4 over a
64 k context (the slots hold K distinct random visible keys, as the indexer fills them); dense: window 128 + every compressed key at
cmp_ratio 128 over a 128 k context (1023 keys).  Every sequence is 37 tokens short of the context.  Per shape both kernels run over several
sets of tables / index rows that name disjoint rows (about 1 GiB of rows where the shape allows it; the report says how much), so consecutive
calls do not find their rows in the last-level cache, and alternate in one process, `rounds` windows each, timed with device events after a
warm-up.

Reported per shape: us per call and the algorithmic bytes per second (sum over tokens of keys x 1024 B for the op; keys x 1152 B for
decode_mla, whose keys carry 64 rope elements) and rate_over_decode_mla, the figure to watch: the aim is >= 1 at B = 128.

Without --only the tool is a driver: every shape runs in a child process of its own under `timeout`, and the first shape that fails ends
the run (nothing more is started on the GPU).  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgl-kernel-npu_amd", "python"))
import torch

HBM_PEAK = 8.0e12
BLOCK, HEADS, D, WIN = 128, 64, 512, 128
SHAPES = ([(f"sparse_k{K}_b{B}", "sparse", B, K, 4, 65536) for K in (512, 1024) for B in (1, 32, 128)]
          + [(f"dense_r128_b{B}", "dense", B, 0, 128, 131072) for B in (1, 32, 128)])
CHILD_TIMEOUT_S = 170


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def bench_shape(name, kind, B, K, ratio, ctx, seed, rounds):
    import sgl_kernel_npu  # noqa: F401
    dtype, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(seed)
    L = ctx - 37
    limit = L // ratio
    ncmp = K if kind == "sparse" else limit
    keys = WIN + ncmp
    read_bytes = B * keys * D * 2
    sets = int(min(64, max(2, -(-(1 << 30) // read_bytes))))
    if kind == "sparse":
        sets = min(sets, limit // K)                                    # the sets name disjoint rows of a sequence's compressed cache
    # original cache: only the two pages under the window are ever read; every other table entry names page 0
    cols = -(-ctx // BLOCK)
    ori = torch.empty((1 + sets * B * 2, BLOCK, 1, D), dtype=dtype, device=dev).normal_(generator=g)
    ori_tables = torch.zeros((sets, B, cols), dtype=torch.int32, device=dev)
    first = (L - WIN) // BLOCK
    own = (1 + torch.randperm(sets * B * 2, generator=g, device=dev)).to(torch.int32).reshape(sets, B, 2)
    ori_tables[:, :, first:first + 2] = own
    # compressed cache: sparse reads K random rows of one big cache per sequence (each set of index rows names other rows); dense reads
    # every row of a cache of its own per set
    cmp_cols = -(-(ctx // ratio) // BLOCK)
    cmp_sets = 1 if kind == "sparse" else sets
    cmp = torch.empty((cmp_sets * B * cmp_cols, BLOCK, 1, D), dtype=dtype, device=dev).normal_(generator=g)
    cmp_tables = torch.randperm(cmp_sets * B * cmp_cols, generator=g, device=dev).to(torch.int32).reshape(cmp_sets, B, cmp_cols)
    idx = None
    if kind == "sparse":
        assert sets * K <= limit
        perm = torch.stack([torch.randperm(limit, generator=g, device=dev)[:sets * K] for _ in range(B)])      # [B, sets * K], distinct per sequence
        idx = perm.reshape(B, sets, K).transpose(0, 1).contiguous().to(torch.int32).reshape(sets, B, 1, 1, K)
    q = (0.1 * torch.randn((B, 1, HEADS, D), generator=g, device=dev) + 0.05).to(dtype)
    sinks = 2.0 * torch.randn((HEADS,), generator=g, device=dev)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    scale = D ** -0.5

    def run_op(i):
        s = i % sets
        return torch.ops.npu.sparse_attn_sharedkv(q, ori_kv=ori, cmp_kv=cmp, cmp_sparse_indices=None if idx is None else idx[s],
                                                  ori_block_table=ori_tables[s], cmp_block_table=cmp_tables[s % cmp_sets], seqused_kv=lens,
                                                  sinks=sinks, softmax_scale=scale, cmp_ratio=ratio, ori_win_left=WIN - 1, ori_win_right=0)[0]

    # comparator: decode_mla, 64 heads, the same number of keys, contiguous pages
    mcols = -(-keys // BLOCK)
    kn = torch.empty((sets * B * mcols, BLOCK, 1, D), dtype=dtype, device=dev).normal_(generator=g)
    kr = torch.empty((sets * B * mcols, BLOCK, 1, 64), dtype=dtype, device=dev).normal_(generator=g)
    mtables = torch.arange(sets * B * mcols, dtype=torch.int32, device=dev).reshape(sets, B, mcols)
    mq = (0.1 * torch.randn((B, HEADS, D + 64), generator=g, device=dev)).to(dtype)
    mout = torch.empty((B, HEADS, D), dtype=dtype, device=dev)
    mlens = torch.full((B,), keys, dtype=torch.int32, device=dev)

    def run_mla(i):
        torch.ops.npu.decode_mla(mq, kn, kr, mout, mlens, scale, BLOCK, mtables[i % sets], 0)

    variants = {"op": run_op, "decode_mla": run_mla}
    out = run_op(0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    for fn in variants.values():
        for i in range(2 * sets):
            fn(i)
    torch.cuda.synchronize()
    calls = {label: int(min(2000, max(5, 50e3 / window(fn, 5)))) for label, fn in variants.items()}      # windows of about 50 ms
    times = {label: [] for label in variants}
    for _ in range(rounds):
        for label, fn in variants.items():
            times[label].append(window(fn, calls[label]))
    nbytes = {"op": B * keys * D * 2, "decode_mla": B * keys * (D + 64) * 2}
    res = dict(shape=dict(kind=kind, B=B, S1=1, context=ctx, cmp_ratio=ratio, window=WIN, sparse_count=K, keys_per_token=keys, block=BLOCK,
                          dtype="bfloat16"), sets_rotated=sets, rotation_working_set_bytes=read_bytes * sets)
    for label, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[label] = dict(median_us=med, min_us=ts[0], max_us=ts[-1], calls_per_window=calls[label], windows=rounds, algorithmic_bytes=nbytes[label],
                          bytes_per_s=nbytes[label] / (med * 1e-6), share_of_hbm_peak=nbytes[label] / (med * 1e-6) / HBM_PEAK)
    res["rate_over_decode_mla"] = res["op"]["bytes_per_s"] / res["decode_mla"]["bytes_per_s"]
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
        out = dict(hbm_peak_bytes_per_s=HBM_PEAK, timing="device events, per-call time of a window", tool="tools/bench_sparse_sharedkv.py",
                   comparator="decode_mla, 64 q heads / 1 kv head, contiguous pages of 128, the same number of keys, measured in the same run",
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
                print(name, json.dumps(child["result"]["rate_over_decode_mla"]), file=sys.stderr, flush=True)
        at128 = [s["rate_over_decode_mla"] for s in out["shapes"].values() if s["shape"]["B"] == 128]
        if at128:
            out["rate_over_decode_mla_at_b128_min"] = min(at128)
            out["aim_met_at_b128"] = all(r >= 1.0 for r in at128)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    if "stopped" in out:
        sys.exit(1)


if __name__ == "__main__":
    main()
