"""compressor (torch.ops.npu.compressor) against the vendor GEMM for its two projections at the same shapes on the same GPU.

bf16, TH layout, paged state (pages of 128).  Prefill: T = 8192 tokens of one sequence from position 0; decode: B = 128 sequences of one
token at start_pos = 8192.  H in {4096, 7168}; (cmp_ratio, coff, D) = (4, 2, 512) and (128, 1, 512).  Every timed call starts behind a
512 MB fill that pushes the weights and the state out of the last-level cache; the call alone sits between two device events; warm-up
calls come first.  The comparator, `torch.matmul(x, wkv.T)` + `torch.matmul(x, wgate.T)`, is timed the same way in the same process.

Reported per shape: median us of the op and of the two matmuls; for prefill the aim `matmul + workspace write and read at the HBM rate
DESIGN.md measures (6.2 TB/s)`; for decode the weight bytes over the op's time against the byte rate of mla_preprocess's skinny GEMMs
(2.7 TB/s).  Aims are reported, not asserted.

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

HBM_RATE = 6.2e12            # the practical ceiling DESIGN.md measures
SKINNY_GEMM_RATE = 2.7e12    # mla_preprocess's per-head skinny GEMM
BLOCK = 128
MODES = {"c4a": (4, 2, 512), "c128a": (128, 1, 512)}
SHAPES = [(f"{kind}_h{H}_{mode}", kind, H, mode) for kind in ("prefill", "decode") for H in (4096, 7168) for mode in MODES]
CHILD_TIMEOUT_S = 120


def bench_shape(name, kind, H, mode, seed, rounds):
    import sgl_kernel_npu  # noqa: F401
    dtype, dev = torch.bfloat16, "cuda"
    r, coff, D = MODES[mode]
    ww = coff * D
    g = torch.Generator(device=dev).manual_seed(seed)
    B, T, start = (1, 8192, 0) if kind == "prefill" else (128, 128, 8192)
    span = T // B
    x = (0.02 * torch.randn((T, H), generator=g, device=dev)).to(dtype)
    wkv = (0.02 * torch.randn((ww, H), generator=g, device=dev)).to(dtype)
    wgate = (0.02 * torch.randn((ww, H), generator=g, device=dev)).to(dtype)
    ape = 0.01 * torch.randn((r, ww), generator=g, device=dev)
    nw = 1.0 + 0.02 * torch.randn((D,), generator=g, device=dev)
    rows = min(T, T // r + B)
    sin = 0.01 * torch.randn((rows, 64), generator=g, device=dev)
    cos = 1.0 + 0.01 * torch.randn((rows, 64), generator=g, device=dev)
    cols = -(-(start + span) // BLOCK)
    first = max(start - coff * r, 0) // BLOCK                                   # only the pages a call touches are backed; the rest name block 0
    table = torch.zeros((B, cols), dtype=torch.int32, device=dev)
    table[:, first:] = (1 + torch.randperm(B * (cols - first), generator=g, device=dev)).to(torch.int32).reshape(B, cols - first)
    state = 0.01 * torch.randn((1 + B * (cols - first), BLOCK, 2 * ww), generator=g, device=dev)
    cu = torch.arange(0, T + 1, span, dtype=torch.int32, device=dev)
    used = torch.full((B,), span, dtype=torch.int32, device=dev)
    pos = torch.full((B,), start, dtype=torch.int32, device=dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def run_op():
        return torch.ops.npu.compressor(x, wkv, wgate, state, ape, nw, sin, cos, state_block_table=table, cu_seqlens=cu, seqused=used,
                                        start_pos=pos, rope_head_dim=64, cmp_ratio=r, coff=coff, norm_eps=1e-6, rotary_mode=2, cache_mode=1)

    def run_matmul():
        return torch.matmul(x, wkv.T), torch.matmul(x, wgate.T)

    def timed(fn):
        flush.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    variants = {"op": run_op, "matmul": run_matmul}
    out = run_op()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    times = {k: [] for k in variants}
    for k, fn in variants.items():
        for _ in range(3):
            timed(fn)
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    weight_bytes = 2 * ww * H * 2
    slab_bytes = T * 2 * ww * 4
    res = dict(shape=dict(kind=kind, T=T, B=B, start_pos=start, hidden=H, cmp_ratio=r, coff=coff, head_dim=D, dtype="bfloat16", cache_mode=1,
                          block_size=BLOCK), weight_bytes=weight_bytes, flops=2 * T * 2 * ww * H)
    for k, ts in times.items():
        ts = sorted(ts)
        res[k] = dict(median_us=ts[len(ts) // 2], min_us=ts[0], max_us=ts[-1], calls=rounds)
    op, mm = res["op"]["median_us"], res["matmul"]["median_us"]
    res["op_over_matmul"] = op / mm
    res["op_tflops"] = res["flops"] / (op * 1e-6) / 1e12
    if kind == "prefill":
        aim = mm + 2 * slab_bytes / HBM_RATE * 1e6
        res["aim_us"] = aim
        res["aim"] = "matmul + workspace write and read at 6.2 TB/s"
    else:
        res["weight_bytes_per_s"] = weight_bytes / (op * 1e-6)
        aim = weight_bytes / SKINNY_GEMM_RATE * 1e6
        res["aim_us"] = aim
        res["aim"] = "weight bytes at 2.7 TB/s"
    res["aim_met"] = op <= aim
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--only", default=None, help="one shape name, measured in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    by_name = {s[0]: s for s in SHAPES}
    if a.only:
        assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
        torch.cuda.set_device(0)
        out = dict(device=torch.cuda.get_device_name(0), result=bench_shape(*by_name[a.only], a.seed, a.rounds))
    else:
        out = dict(timing="device events around one call, each behind a 512 MB cache flush; median", tool="tools/bench_compressor.py",
                   comparator="torch.matmul(x, wkv.T) and torch.matmul(x, wgate.T), measured in the same process", shapes={})
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
                print(name, child["result"]["op"]["median_us"], child["result"]["matmul"]["median_us"], file=sys.stderr, flush=True)
        out["aims_met"] = {n: s["aim_met"] for n, s in out["shapes"].items()}
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    if "stopped" in out:
        sys.exit(1)


if __name__ == "__main__":
    main()
