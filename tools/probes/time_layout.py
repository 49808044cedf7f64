"""Scratch: dispatch layout at C2 size (4096 tokens, top-8 of 256, 8 ranks) and around it: three launches vs the cooperative single
launch, back to back on one stream.

  python tools/probes/time_layout.py [--lib PATH]      (default: the built libmi_ep.so)"""
import argparse, ctypes, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch
from capi import ptr, stream_ptr
from ctypes import c_int, c_size_t, c_void_p

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "sgl-kernel-npu_amd", "lib", "libmi_ep.so"))
a = ap.parse_args()
L = ctypes.CDLL(a.lib)
V, I = c_void_p, c_int
L.mi_ep_dispatch_layout.argtypes = [V, I, I, I, I, I, V, V, V, V, V, V, c_size_t, V, V, V]
L.mi_ep_dispatch_layout_workspace.restype = c_size_t
L.mi_ep_dispatch_layout_workspace.argtypes = [I, I, I]
print("lib:", os.path.relpath(a.lib, ROOT))
for T, W in ((1024, 8), (1025, 8), (4096, 8), (4096, 1), (16384, 8)):
    E, K = 256, 8
    idx = torch.topk(torch.rand((T, E), device="cuda"), K, dim=-1)[1]
    i32 = dict(dtype=torch.int32, device="cuda")
    o = [torch.empty(W, **i32), torch.empty(E, **i32), torch.empty((T, W), **i32), torch.empty((T, K), **i32), torch.empty(E, **i32)]
    wsb = L.mi_ep_dispatch_layout_workspace(T, K, E)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    words = torch.zeros(2, **i32)
    args = [ptr(idx), 0, T, K, E, W] + [ptr(t) for t in o] + [ptr(ws), wsb]
    for coop in (False, True):
        call = lambda: L.mi_ep_dispatch_layout(*args, ptr(words) if coop else None, None, stream_ptr())
        for _ in range(20): call()
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record()
            for _ in range(200): call()
            b_.record(); torch.cuda.synchronize()
            per.append(a_.elapsed_time(b_) / 200 * 1e3)
        print(f"T={T} W={W} {'one launch    ' if coop else 'three launches'}: {min(per):.2f}-{max(per):.2f} us per call over 5 x 200 "
              f"(back to back, outputs preallocated)", flush=True)
