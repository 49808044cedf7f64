"""Single-rank dispatch in one launch (mi_ep_dispatch_stage_local_tables): workgroup 0 builds the W = 1 count tables, the host summary
and the call counter step that mi_ep_notify_tables does, and the token workgroups write the bytes of mi_ep_dispatch_stage_local --
checked bit for bit against those two launches, and through deep_ep.Buffer with the switch on and off."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed

import ep_harness as Hh
import mp_workers
from capi import ptr, stream_ptr
from test_deep_ep_plumbing_cpu import _spawn, free_port

pytestmark = pytest.mark.gpu

TABLES = ("cnt", "recv_count", "recv_offset", "recv_tokens_per_expert", "expert_global_offset", "srcrank_in_expert_offset",
          "r_in_srcrank_offset", "total_recv_token", "max_bs", "pull_offset")


def _lib():
    lib = Hh.lib()
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.mi_ep_dispatch_stage_local.argtypes = [V, V, I, V, V, V, I, I, I, I, I, I, V, V, V, V, V]
    lib.mi_ep_dispatch_stage_local.restype = ctypes.c_int
    lib.mi_ep_dispatch_stage_local_tables.argtypes = [V, V, I, V, V, I, I, I, I, I, I, V, V, V, V, I] + [V] * 13
    lib.mi_ep_dispatch_stage_local_tables.restype = ctypes.c_int
    lib.mi_ep_notify_tables.argtypes = [V, I, I, I, I] + [V] * 11
    lib.mi_ep_notify_tables.restype = ctypes.c_int
    return lib


def _payload_bytes(H, qm):
    return H * 2 if qm == Hh.QUANT_NONE else (H // 2 if qm == 6 else H)


def _outputs(rows, T, K, H, E, qm):
    """Sentinel-filled outputs: bytes neither form writes must stay equal too."""
    d = "cuda"
    o = dict(rx=torch.full((rows, _payload_bytes(H, qm)), 0x5A, dtype=torch.uint8, device=d),
             tri=torch.full((rows * 3,), -9, dtype=torch.int32, device=d),
             lro=torch.full((max(T * K, 1),), -7, dtype=torch.int32, device=d))
    if qm in (4, 5, 6):
        o["rs"] = torch.full((rows * (H // 32),), 0x33, dtype=torch.uint8, device=d)
    elif qm != Hh.QUANT_NONE:
        o["rs"] = torch.full((rows,), -3.0, dtype=torch.float32, device=d)
    else:
        o["rs"] = None
    for k in TABLES:
        n = {"cnt": E + 1, "total_recv_token": 1, "max_bs": 1}.get(k, E)
        o[k] = torch.full((n,), -5, dtype=torch.int32, device=d)
    o["summary"] = torch.full((2 + E,), -1, dtype=torch.int32, device=d)
    o["ctr"] = torch.tensor([41], dtype=torch.int64, device=d)
    return o


def _tables_args(o):
    return [ptr(o[k]) for k in TABLES] + [ptr(o["summary"]), ptr(o["ctr"])]


def _both_forms(idx, E, qm, H, rows_hint=None, seed=0):
    lib = _lib()
    T, K = idx.shape
    rng = np.random.default_rng(seed)
    from oracle.bf16 import f32_to_bf16_bits_rne
    x = torch.from_numpy(f32_to_bf16_bits_rne((rng.standard_normal((T, H)) * 2).astype(np.float32)).view(np.int16)).cuda()
    ti = torch.from_numpy(idx).cuda()
    lay = Hh.layout(ti, E, 1)
    cnt = lay["num_tokens_per_expert"]
    R = int(cnt.sum().item())
    hint = max(R, 1) if rows_hint is None else rows_hint
    rows = max(T * K, 1)
    i32 = int(ti.dtype == torch.int32)
    st = stream_ptr()
    ref, got = _outputs(rows, T, K, H, E, qm), _outputs(rows, T, K, H, E, qm)
    # reference: the count row, notify_tables (W = 1) and stage_local, the counter moved on by hand as the notify launch does
    ref["cnt"][:E] = cnt
    ref["cnt"][E] = T
    Hh.ck(lib.mi_ep_notify_tables(ptr(ref["cnt"]), 1, E, 0, 0, *[ptr(ref[k]) for k in TABLES[1:]], ptr(ref["summary"]), st))
    ref["ctr"] += 1
    if T:
        Hh.ck(lib.mi_ep_dispatch_stage_local(ptr(x), ptr(ti), i32, ptr(lay["send_token_idx_small"]), ptr(ref["recv_count"]), ptr(cnt),
                                             T, K, H, E, qm, hint, ptr(ref["rx"]), ptr(ref["rs"]), ptr(ref["tri"]), ptr(ref["lro"]), st))
    Hh.ck(lib.mi_ep_dispatch_stage_local_tables(ptr(x), ptr(ti), i32, ptr(lay["send_token_idx_small"]), ptr(cnt), T, K, H, E, qm, hint,
                                                ptr(got["rx"]), ptr(got["rs"]), ptr(got["tri"]), ptr(got["lro"]), 0, *_tables_args(got), st))
    torch.cuda.synchronize()
    return ref, got


def _assert_same(ref, got, what):
    for k, v in ref.items():
        if v is not None:
            assert torch.equal(v, got[k]), (k, what)


def _topk(rng, T, K, E, i32):
    idx = mp_workers.make_topk(rng, T, K, E, 0.1) if T else np.zeros((0, K), np.int64)
    if T > 1:
        idx[1, :] = -1                       # a token that selects nothing
    if T > 5:
        idx[5, 1] = -1
    return idx.astype(np.int32) if i32 else idx


@pytest.mark.parametrize("T", [0, 1, 300, 4096, 16384])
@pytest.mark.parametrize("E", [8, 256, 2048])
def test_stage_local_tables_matches_notify_tables_and_stage_local(T, E):
    """Every quant mode, int32 and int64 ids: tables, count row, summary words, counter, rows, scales, triples and local_row_out."""
    K = min(8, E)
    H = 7168 if T <= 4096 else 2048
    rng = np.random.default_rng(10 * T + E)
    for i32 in (False, True):
        idx = _topk(rng, T, K, E, i32)
        for qm in range(7):
            _assert_same(*_both_forms(idx, E, qm, H, seed=T + E + qm), (T, E, qm, i32))


def test_stage_local_tables_rows_hint_below_total():
    E, K, T, H = 256, 8, 300, 1024
    idx = _topk(np.random.default_rng(3), T, K, E, False)
    for qm in (0, 1, 4):
        _assert_same(*_both_forms(idx, E, qm, H, rows_hint=700), ("hint", qm))
        _assert_same(*_both_forms(idx, E, qm, H, rows_hint=0), ("hint0", qm))


def test_stage_local_tables_rejects_bad_arguments():
    lib = _lib()
    i32 = torch.zeros(4096, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()
    x = torch.zeros((4, 64), dtype=torch.bfloat16, device="cuda")
    ti = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    tb = [ptr(i32)] * 10 + [None, ptr(ctr)]
    call = lambda H, qm, E=8, xp=ptr(x), tbl=tb: lib.mi_ep_dispatch_stage_local_tables(
        xp, ptr(ti), 0, ptr(i32), ptr(i32), 4, 2, H, E, qm, 8, ptr(i32), None, ptr(i32), None, 0, *tbl, st)
    assert call(72, 1) != 0                         # H % 16
    assert call(64, 7) != 0                         # unknown quant mode
    assert call(64, 1, E=4096) != 0                 # E > 2048
    assert call(64, 1, xp=ctypes.c_void_p(0)) != 0  # missing x
    assert call(64, 1, tbl=[None] + tb[1:]) != 0    # missing count row
    assert call(64, 1) == 0
    torch.cuda.synchronize()


# ---- through deep_ep.Buffer at W = 1: the switch on and off ------------------------------------------------------------------------
def _buffer_worker(rank, world, port, cfg):
    mp_workers.run_guarded(_buffer_forms, rank, world, port, cfg)


def _buffer_forms(rank, world, port, cfg):
    import deep_ep
    from oracle.bf16 import bits_to_torch
    mp_workers._set_device(rank)
    quant, capture = cfg
    group = mp_workers._init(rank, world, port)
    E, K, H, T_max = 256, 8, 7168, 4096
    os.environ["DEEPEP_WINDOW_BYTES"] = str(6 * (T_max * K * H * 2 + (8 << 20)) + (4 << 20))
    buf = deep_ep.Buffer(group, low_latency_mode=True)
    assert buf.runtime.get_dispatch_local_tables()          # on by default
    stats = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(x, ti, tw, worst=0, with_stats=False):
        per_rank, _, per_expert, is_in, _ = buf.get_dispatch_layout(ti, E)
        rx, _, _, lst, handle, _ = buf.dispatch(x, num_tokens_per_rank=per_rank, is_token_in_rank=is_in, num_tokens_per_expert=per_expert,
                                                topk_idx=ti, topk_weights=tw, quant_mode=quant, num_worst_tokens=worst,
                                                dispatch_wait_recv_cost_stats=stats if with_stats else None)
        rx, rs = rx if quant else (rx, None)
        y = (rx.float() * rs[:, None]).to(torch.bfloat16) if quant else rx
        out, _, _ = buf.combine(y, handle)
        return [rx.view(torch.uint8) if quant else rx, rs, handle[3], out], lst

    def same(u, v, n):
        """rx, scales, triples: the n received rows (a call that receives nothing returns one unwritten row); combine: all of it."""
        rows = [n, n, 3 * n, None]
        return all(a is None or torch.equal(a[:m] if m is not None else a, b[:m] if m is not None else b) for a, b, m in zip(u, v, rows))

    def inputs(T, seed):
        xs, idxs, ws = mp_workers.make_inputs(1, T, H, K, E, 0.1, seed=seed)
        idx = idxs[0][:T]
        idx[min(7, T - 1), :] = -1
        return bits_to_torch(xs[0][:T]).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(np.abs(ws[0][:T])).cuda()

    # the very first call of the Buffer takes the one-launch form (no speculative guess needed)
    for it, T in enumerate((300, T_max, 1, T_max)):
        x, ti, tw = inputs(T, 700 + it)
        res = {}
        for on in (True, False, True, False):
            buf.runtime.set_dispatch_local_tables(on)
            buf.begin_profile(0, 1, "")
            got, lst = run(x, ti, tw)
            buf.end_profile()
            names = {k for k, (n, _) in buf.get_profile_summary().items() if n}
            assert "dispatch_stage_local" in names and ("dispatch_notify" in names) == (not on), names
            if on in res:
                assert res[on][1] == lst and same(res[on][0], got, sum(lst)), (T, on)
            res[on] = (got, lst)
        (a, la), (b, lb) = res[False], res[True]
        assert la == lb
        n = sum(lb)
        assert same(a, b, n), (T,)
        # wait statistics asked for: the notify launch runs (the only place that measures the wait), same results
        buf.runtime.set_dispatch_local_tables(True)
        buf.begin_profile(0, 1, "")
        got, lst = run(x, ti, tw, with_stats=True)
        buf.end_profile()
        assert "dispatch_notify" in {k for k, (n_, _) in buf.get_profile_summary().items() if n_}
        assert lst == lb and same(b, got, n)
        # num_worst_tokens: worst-case sized outputs, no host sync
        wres = {}
        for on in (True, False):
            buf.runtime.set_dispatch_local_tables(on)
            wres[on], lw = run(x, ti, tw, T * K)
            assert lw == []
        (ux, us, ui, uo), (vx, vs, vi, vo) = wres[False], wres[True]
        assert torch.equal(ux[:n], vx[:n]) and torch.equal(ui[:3 * n], vi[:3 * n]) and torch.equal(uo, vo)
        assert us is None or torch.equal(us[:n], vs[:n])
        assert torch.equal(vo, b[3])
    buf.runtime.set_dispatch_local_tables(True)
    if capture:
        # the num_worst_tokens one-launch form captured in a graph, replayed between eager calls of both forms (the call counter)
        T = 512
        x_s = torch.zeros((T, H), dtype=torch.bfloat16, device="cuda")
        ti_s = torch.zeros((T, K), dtype=torch.int64, device="cuda")
        tw_s = torch.zeros((T, K), dtype=torch.float32, device="cuda")

        def load(seed):
            x, ti, tw = inputs(T, seed)
            x_s.copy_(x), ti_s.copy_(ti), tw_s.copy_(tw)

        load(1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                run(x_s, ti_s, tw_s, T * K)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap, _ = run(x_s, ti_s, tw_s, T * K)
        for rep in range(2):
            load(300 + rep)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for on, worst in ((True, 0), (False, 0), (False, T * K), (True, T * K)):
                buf.runtime.set_dispatch_local_tables(on)
                eager, _ = run(x_s, ti_s, tw_s, worst)
                torch.cuda.synchronize()
                n = int((ti_s >= 0).sum().item())
                assert torch.equal(cap[0][:n], eager[0][:n]) and torch.equal(cap[2][:3 * n], eager[2][:3 * n]), (rep, on, worst)
                if quant:
                    assert torch.equal(cap[1][:n], eager[1][:n]), (rep, on, worst)
                assert torch.equal(cap[3], eager[3]), (rep, on, worst)
            buf.runtime.set_dispatch_local_tables(True)
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("cfg", [(None, False), ("int8", True)], ids=["bf16", "int8_graph"])
def test_buffer_dispatch_with_and_without_local_tables(cfg):
    _spawn(_buffer_worker, 1, cfg)


def test_buffer_dispatch_local_tables_without_speculation():
    """DEEPEP_SPECULATIVE_RECV=0 (read once per process, so in a fresh child): the host-synced call keeps the notify launch, and the
    results equal the one-launch form's."""
    code = r"""
import os, sys
import torch, numpy as np
sys.path[:0] = [os.environ["MI_ROOT"], os.path.join(os.environ["MI_ROOT"], "tests")]
from test_dispatch_local_tables_gpu import _child_main
_child_main()
"""
    root = mp_workers.ROOT
    env = dict(os.environ, DEEPEP_SPECULATIVE_RECV="0", MI_ROOT=root,
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.path.join(root, "sgl-kernel-npu_amd", "python"),
                                           os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _child_main():
    import deep_ep
    from oracle.bf16 import bits_to_torch
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(free_port()))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=0, world_size=1)
    E, K, H, T = 256, 8, 7168, 1024
    buf = deep_ep.Buffer(torch.distributed.group.WORLD, low_latency_mode=True)
    xs, idxs, ws = mp_workers.make_inputs(1, T, H, K, E, 0.1, seed=9)
    x, ti, tw = bits_to_torch(xs[0][:T]).cuda(), torch.from_numpy(idxs[0][:T]).cuda(), torch.from_numpy(np.abs(ws[0][:T])).cuda()
    outs = {}
    for on in (True, False):
        buf.runtime.set_dispatch_local_tables(on)
        per_rank, _, per_expert, is_in, _ = buf.get_dispatch_layout(ti, E)
        buf.begin_profile(0, 1, "")
        (rx, rs), _, _, lst, handle, _ = buf.dispatch(x, num_tokens_per_rank=per_rank, is_token_in_rank=is_in,
                                                      num_tokens_per_expert=per_expert, topk_idx=ti, topk_weights=tw, quant_mode="int8")
        buf.end_profile()
        names = {k for k, (n, _) in buf.get_profile_summary().items() if n}
        assert "dispatch_notify" in names, names             # no speculation: the host-synced call keeps the notify launch
        outs[on] = (rx.clone(), rs.clone(), handle[3].clone(), lst)
    a, b = outs[True], outs[False]
    assert a[3] == b[3] and all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))
    torch.cuda.synchronize()
    torch.distributed.destroy_process_group()
