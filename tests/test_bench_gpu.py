"""bench.py contract: the launch line the driver uses for N > 1, exercised on ONE GPU (every rank on cuda:0, gloo bootstrap --
BENCH_SINGLE_DEVICE=1), the plain N = 1 run (the headline alone) and the N = 1 run with --full (every section).  The JSON object must
be the LAST line of stdout."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")


def _last_json(stdout):
    lines = [l for l in stdout.strip().splitlines() if l.strip()]
    assert lines, "bench.py printed nothing"
    return json.loads(lines[-1])          # must parse: nothing may follow the JSON line


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_two_ranks_one_gpu():
    env = dict(os.environ, BENCH_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    # plain `python bench.py --gpus 2`, no RANK in the environment: bench.py re-executes itself through torch.distributed.run (the
    # launch line the driver uses for N > 1), so this one call covers the self-launch AND the launcher form
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["strategy"] == "default" and d["validated_round_trip"] is True
    # N > 1: the top-level roofline is the link-facing leg (the HBM-side kernel of the N = 1 line rides along as `hbm_side`)
    rf = d["roofline"]
    assert rf["bound"] == "xgmi" and rf["unit"] == "GB/s" and rf["peak"] > 0 and rf["achieved"] > 0 and 0 < rf["frac"]
    assert rf["kernel"] in ("combine_push", d["xgmi"]["dispatch_kernel"]) and rf["hbm_side"]["bound"] == "hbm"
    # N > 1: both dispatch transports timed with the same K steps, the cross-GPU legs priced per leg and per link, C3 / C5 emitted
    assert set(d["transports"]) == {"push", "pull"} and d["config"]["dispatch_transport"] in ("push", "pull")
    assert {"dispatch_frac", "combine_frac", "dispatch_max_link_bytes", "combine_max_link_bytes"} <= set(d["xgmi"])
    assert d["low_latency"]["validated_round_trip"] is True and d["low_latency"]["dispatch_us_p50"] > 0
    assert d["fused_deep_moe"].get("validated") is True and d["fused_deep_moe"]["validation"]["avg_diff_max"] < 4e-4, d["fused_deep_moe"]


FULL_ONLY = ("roofline", "kernels", "profiled_ms_per_step", "no_host_sync", "ep8_proxy", "xgmi_projection", "low_latency", "fused_deep_moe",
             "mla_decode", "cpu_baseline")
PLAIN_SECONDS_OUTSIDE_STEPS = 30.0


def _check_dumped_outputs(directory):
    # --dump-outputs: the last timed step's outputs, float32 / float64, within 64 MB; the sampled combined rows are the round trip's
    import numpy as np
    got = {f[:-4]: np.load(directory / f) for f in os.listdir(directory)}
    assert set(got) == {"num_tokens_per_rank", "num_tokens_per_expert", "is_token_in_rank", "num_recv_tokens_per_expert", "recv_x",
                        "recv_x_scales", "combined_x"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    n = int(got["num_recv_tokens_per_expert"].sum())
    assert got["num_tokens_per_rank"].tolist() == [4096] and got["recv_x_scales"].shape == (n,)
    assert got["recv_x"].shape == (512, 7168) and got["combined_x"].shape == (512, 7168) and np.isfinite(got["combined_x"]).all()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_plain_run_is_lean(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline keys and the dumped outputs, none of the sections that
    take runs of their own, and at most 30 s of the whole run -- a new process, from start to exit -- outside its K + W steps."""
    steps, warmup = 30, 5
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=540)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "int8/bf16" and d["vs_baseline"] is None
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["validated_round_trip"] is True and d["config"]["strategy"] == "default"
    assert not set(FULL_ONLY) & set(d), sorted(set(FULL_ONLY) & set(d))
    _check_dumped_outputs(tmp_path)
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s in all, {outside:.2f} s outside its {steps} + {warmup} steps of {d['ms_per_step']:.4f} ms")
    assert outside <= PLAIN_SECONDS_OUTSIDE_STEPS, outside


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_single_gpu_line(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-mla",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["full"] is True
    for k in REQUIRED + ("roofline", "cpu_baseline", "low_latency", "fused_deep_moe"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["dtype"] == "int8/bf16" and d["vs_baseline"] is None
    assert d["cpu_baseline"]["cores"] >= 1 and "single_core" in d["cpu_baseline"]
    assert d["fused_deep_moe"]["roofline"]["bound"] == "mfma" and d["fused_deep_moe"]["validated"] is True
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source")) <= set(d["roofline"])
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(d["cpu_baseline"])
    # the number that transfers to EP = 8: every row through the window paths, kernel by kernel
    px = d["ep8_proxy"]
    assert px["ms_per_step"] > d["ms_per_step"] and {"dispatch_pull", "combine_push", "combine_reduce"} <= set(px["kernels"])
    assert px["kernels"]["combine_push"]["algorithmic_bytes"] > 9e8
    # the stated expectation for the first EP = 8 run: per-leg cross-GPU bytes, link-bound time, projected step
    xp = d["xgmi_projection"]
    assert xp["ep"] == 8 and xp["peak_GBps"] == 7 * 153.0 and set(xp["legs"]) == {"dispatch_push", "combine_push"}
    assert xp["legs"]["combine_push"]["cross_gpu_bytes"] > 3.5e8 and xp["projected_step_ms"] > xp["link_bound_floor_ms"] > 0.3
    _check_dumped_outputs(tmp_path)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_dry_run_eight_ranks_one_gpu():
    """`bench.py --dry-run-8 --full`: the 8-GPU launch line on ONE GPU at full C2 size (every rank on cuda:0, hipIpc windows): every key a real
    8-GPU line carries must be there -- both transports, per-leg and per-link xGMI pricing, C3 and C5 sections validated."""
    import mp_workers
    if 8 + 1 > mp_workers.MAX_PROCS_PER_GPU:          # eight ranks and this process, all on cuda:0
        pytest.skip(f"needs a GPU that 9 processes may share, at most {mp_workers.MAX_PROCS_PER_GPU} may share one here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run-8", "--full", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=840)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 8 and d["dry_run_single_device"] is True and d["scaling"] == "weak" and d["validated_round_trip"] is True
    assert d["config"]["strategy"] == "default" and d["config"]["tokens_per_rank"] == 4096
    assert set(d["transports"]) == {"push", "pull"}
    xg = d["xgmi"]
    for k in ("peak_GBps", "link_GBps", "dispatch_bytes", "combine_bytes", "dispatch_max_link_bytes", "combine_max_link_bytes",
              "dispatch_GBps", "dispatch_frac", "dispatch_max_link_frac", "combine_GBps", "combine_frac", "combine_max_link_frac"):
        assert k in xg and xg[k] > 0, k
    assert xg["peak_GBps"] == 7 * 153.0
    assert d["low_latency"]["validated_round_trip"] is True and d["fused_deep_moe"]["validated"] is True
    assert "ep8_proxy" in d and "kernels" in d["ep8_proxy"]
