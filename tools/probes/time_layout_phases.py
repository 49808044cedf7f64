"""Scratch: phase timestamps (100 MHz) of the one-launch layout kernel, taken by thread 0 of workgroup 0 (library built with
-DLAYOUT_TIMING: tools/build_timing_ep.sh t -DLAYOUT_TIMING).  Median over --reps launches, each waited for.

  python tools/probes/time_layout_phases.py [--lib PATH] [--names a,b,c,...]

--names: labels of the intervals between consecutive stamps of the cooperative form, for a library whose stamps sit elsewhere."""
import argparse, ctypes, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from capi import ptr, stream_ptr
from ctypes import c_int, c_size_t, c_void_p

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "sgl-kernel-npu_amd", "lib", "timing_ep", "libmi_ep_t.so"))
ap.add_argument("--names", default="init+pass1,totals+local scan+arrive,local pass3,poll,departure,front rows,slots+tables")
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
L = ctypes.CDLL(a.lib)
V, I = c_void_p, c_int
L.mi_ep_dispatch_layout.argtypes = [V, I, I, I, I, I, V, V, V, V, V, V, c_size_t, V, V, V]
L.mi_ep_dispatch_layout.restype = c_int
COOP = a.names.split(",")
SINGLE = ["init+pass1", "-", "pass2", "pass3"]
print("lib:", os.path.relpath(a.lib, ROOT))
# the last shape is the benchmark's own: one rank, int64 ids
for T, W in ((128, 8), (1024, 8), (4096, 8), (16384, 8), (4096, 1)):
    E, K = 256, 8
    idx = torch.topk(torch.rand((T, E), device="cuda"), K, dim=-1)[1]
    assert idx.dtype == torch.int64
    i32 = dict(dtype=torch.int32, device="cuda")
    o = [torch.empty(W, **i32), torch.empty(E, **i32), torch.empty((T, W), **i32), torch.empty((T, K), **i32), torch.empty(E, **i32)]
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    words = torch.zeros(2, **i32)
    rows = []
    for rep in range(a.reps + 5):
        rc = L.mi_ep_dispatch_layout(ptr(idx), 0, T, K, E, W, *[ptr(t) for t in o], ptr(ws), 1 << 20, ptr(words), None, stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        tk = [t for t in ws[512 << 10:(512 << 10) + 64].view(torch.int64).cpu().tolist() if t]
        if rep >= 5:
            rows.append([(tk[i + 1] - tk[i]) / 100 for i in range(len(tk) - 1)])
    assert not words.any()
    n = len(rows[0])
    names = COOP if n == len(COOP) else SINGLE            # lent words: one workgroup only up to 256 tokens
    med = [statistics.median(r[i] for r in rows) for i in range(n)]
    tot = [sum(r) for r in rows]
    print(f"T={T} W={W}: us " + ", ".join(f"{names[i] if i < len(names) else i}={med[i]:.2f}" for i in range(n))
          + f" | total median {statistics.median(tot):.2f} min {min(tot):.2f} max {max(tot):.2f}", flush=True)
