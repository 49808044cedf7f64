"""Single-rank dispatch in one launch (mi_ep_dispatch_stage_local): x quantised straight into the receive rows must produce the
bytes of stage_compact + pull_local -- rows, scales, (src, t, k) triples, local_row_out -- and, through deep_ep.Buffer at W = 1,
the same dispatch and combine results with the switch on and off, both equal to the oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed

import ep_harness as Hh
import mp_workers
from capi import ptr, stream_ptr
from oracle import ep as O
from test_deep_ep_plumbing_cpu import _spawn

pytestmark = pytest.mark.gpu

MODES = {Hh.QUANT_NONE: False, Hh.QUANT_INT8: True, Hh.QUANT_INT8_NOEPS: "noeps", Hh.QUANT_FP8_E4M3: "fp8"}
MAX_HIDDEN = 8192       # MI_EP_MAX_HIDDEN


def _lib():
    lib = Hh.lib()
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.mi_ep_dispatch_stage_local.argtypes = [V, V, I, V, V, V, I, I, I, I, I, I, V, V, V, V, V]
    lib.mi_ep_dispatch_stage_local.restype = ctypes.c_int
    return lib


def _bits(rng, T, H):
    from oracle.bf16 import f32_to_bf16_bits_rne
    return f32_to_bf16_bits_rne((rng.standard_normal((T, H)) * 2).astype(np.float32))


def _topk(rng, T, K, E):
    idx = mp_workers.make_topk(rng, T, K, E, 0.1) if T else np.zeros((0, K), np.int64)
    if T > 1:
        idx[1, :] = -1                       # a token that selects nothing
    return idx


def _both_forms(x_bits, idx, E, qm):
    """-> (unfused, fused): dicts of recv_x bytes, scales, triples and local_row_out, from stage_compact + pull_local and from
    stage_local, on the same layout and the W = 1 count table (recv_count = inclusive cumsum of the per-expert counts)."""
    lib = _lib()
    T, K = idx.shape
    H = x_bits.shape[1]
    x = torch.from_numpy(x_bits.view(np.int16)).cuda()
    ti = torch.from_numpy(idx).cuda()
    lay = Hh.layout(ti, E, 1)
    cnt = lay["num_tokens_per_expert"]
    recv_count = torch.cumsum(cnt, 0, dtype=torch.int32)
    R = int(cnt.sum().item())
    rows = max(R, 1)
    rb = lib.mi_ep_dispatch_row_bytes(H, qm)
    region = torch.zeros(max(T, 1) * (rb + 8 * K) + 4096, dtype=torch.uint8, device="cuda")
    i32idx = int(ti.dtype == torch.int32)
    st = stream_ptr()
    pb = H * (2 if qm == Hh.QUANT_NONE else 1)
    outs = []
    for fused in (False, True):
        # sentinels: bytes neither form writes must stay equal too
        rx = torch.full((rows, pb), 0x5A, dtype=torch.uint8, device="cuda")
        rs = torch.full((rows,), -3.0, dtype=torch.float32, device="cuda") if qm != Hh.QUANT_NONE else None
        tri = torch.full((rows * 3,), -9, dtype=torch.int32, device="cuda")
        lro = torch.full((max(T * K, 1),), -7, dtype=torch.int32, device="cuda")
        if fused:
            Hh.ck(lib.mi_ep_dispatch_stage_local(ptr(x), ptr(ti), i32idx, ptr(lay["send_token_idx_small"]), ptr(recv_count), ptr(cnt),
                                                 T, K, H, E, qm, R, ptr(rx), ptr(rs), ptr(tri), ptr(lro), st))
        else:
            Hh.ck(lib.mi_ep_dispatch_stage_compact(ptr(x), ptr(ti), i32idx, ptr(lay["send_token_idx_small"]), ptr(lay["send_data_offset"]),
                                                   T, K, H, E, 0, qm, ptr(region), region.numel(), None, 0, st))
            Hh.ck(lib.mi_ep_dispatch_pull_local(ptr(region), ptr(ti), i32idx, ptr(lay["send_token_idx_small"]), ptr(recv_count), ptr(cnt),
                                                T, K, H, E, 1, 0, qm, R, ptr(rx), ptr(rs), ptr(tri), ptr(lro), None, 0, st))
        torch.cuda.synchronize()
        outs.append(dict(recv_x=rx, recv_s=rs, tri=tri, local_row=lro, R=R))
    return outs


def _oracle(x_bits, idx, E, qm):
    """-> (payload [R, H] (bf16 bits / int8 / e4m3 bits), scales f32 [R] or None, triples [3R]) in receive-row order."""
    if qm == Hh.QUANT_INT8_NOEPS:       # the receive order of any mode, the rows of the low-latency rounding
        want = O.normal_dispatch([x_bits], [idx], E, False)[0]
        t = want.recv_src_idx.reshape(-1, 3)[:want.total_recv, 1]
        q, s = O.quant_int8_rows(x_bits, None)
        return q[t], s[t], want.recv_src_idx[:3 * want.total_recv]
    want = O.normal_dispatch([x_bits], [idx], E, MODES[qm])[0]
    n = want.total_recv
    return want.recv_x[:n], None if want.recv_x_scales is None else want.recv_x_scales[:n], want.recv_src_idx[:3 * n]


def _check(x_bits, idx, E, qm, bad=None):
    """bad: {token: column} of non-finite elements (their quantised bytes are unspecified by the oracle and not compared to it; the
    FP8 oracle does not model non-finite rows, so those are compared between the two launch forms only)."""
    T, K = idx.shape
    H = x_bits.shape[1]
    ref, got = _both_forms(x_bits, idx, E, qm)
    for k in ("recv_x", "recv_s", "tri", "local_row"):
        if ref[k] is not None:
            assert torch.equal(ref[k], got[k]), (k, qm, T, H)
    n = got["R"]
    if bad and qm == Hh.QUANT_FP8_E4M3:
        return
    wx, ws, wt = _oracle(x_bits, idx, E, qm)
    tri = got["tri"].cpu().numpy()[:3 * n]
    assert np.array_equal(tri, wt)
    gx = got["recv_x"].cpu().numpy()[:n]
    gx = gx.view(np.uint16) if qm == Hh.QUANT_NONE else (gx.view(np.int8) if qm != Hh.QUANT_FP8_E4M3 else gx)
    mask = np.ones((n, H), bool)
    if bad and qm != Hh.QUANT_NONE:
        for j, t in enumerate(tri.reshape(-1, 3)[:, 1]):
            if int(t) in bad:
                mask[j, bad[int(t)]] = False
    assert np.array_equal(gx[mask], wx.view(gx.dtype)[mask]), (qm, T, H)
    if ws is not None:
        assert np.array_equal(got["recv_s"].cpu().numpy()[:n].view(np.uint32), ws.view(np.uint32))
    # local_row_out: every valid selection (t, k) names the receive row holding its (0, t, k) triple
    lro = got["local_row"].cpu().numpy()[:T * K].reshape(T, K) if T else np.zeros((0, K), np.int32)
    valid = idx >= 0
    tr = tri.reshape(-1, 3)
    assert (lro[~valid] == -7).all()
    ts, ks = np.nonzero(valid)
    assert np.array_equal(tr[lro[ts, ks]], np.stack([np.zeros_like(ts), ts, ks], 1).astype(np.int32))


@pytest.mark.parametrize("H", [16, 7168, MAX_HIDDEN])
@pytest.mark.parametrize("T", [0, 1, 131, 4096])
def test_stage_local_matches_stage_and_pull_local(T, H):
    """Every quant mode, int32 and int64 topk_idx: identical bytes to the two-launch form, and the oracle's rows."""
    E, K = 256, 8
    rng = np.random.default_rng(1000 + T + H)
    x_bits = _bits(rng, T, H)
    idx = _topk(rng, T, K, E)
    for qm in MODES:
        for i32 in (False, True):
            _check(x_bits, idx.astype(np.int32) if i32 else idx, E, qm)


def test_stage_local_non_finite_rows():
    """Rows holding NaN / inf quantise as stage_int8 does (amax = inf -> scale inf, finite elements 0), as in test_ep_fuzz_gpu."""
    E, K, T, H = 64, 4, 131, 7168
    rng = np.random.default_rng(77)
    x_bits = _bits(rng, T, H)
    bad = {3: 17, 5: 900, 9: 0, 11: 513}
    x_bits[3, 17], x_bits[5, 900], x_bits[9, 0], x_bits[11, 513] = 0x7FC0, 0xFFFF, 0x7F80, 0xFF80
    idx = _topk(rng, T, K, E)
    idx[3:12, 0] = np.arange(9) % E                # the bad tokens are all received
    for qm in MODES:
        _check(x_bits, idx, E, qm, bad)


def test_stage_local_rejects_bad_arguments():
    lib = _lib()
    x = torch.zeros((4, 64), dtype=torch.bfloat16, device="cuda")
    ti = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    rx = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    st = stream_ptr()
    call = lambda H, qm, xp=ptr(x): lib.mi_ep_dispatch_stage_local(xp, ptr(ti), 0, ptr(i32), ptr(i32), ptr(i32), 4, 2, H, 8, qm, 8,
                                                                    ptr(rx), None, ptr(i32), None, st)
    assert call(MAX_HIDDEN + 16, 1) != 0            # the row lives in registers: no hidden size beyond MI_EP_MAX_HIDDEN
    assert call(72, 1) != 0                         # H % 16
    assert call(64, 7) != 0                         # unknown quant mode
    assert call(64, 1, ctypes.c_void_p(0)) != 0     # missing x
    assert call(64, 1) == 0
    torch.cuda.synchronize()


# ---- through deep_ep.Buffer at W = 1: the switch on and off ------------------------------------------------------------------------
def _buffer_worker(rank, world, port, cfg):
    mp_workers.run_guarded(_buffer_both_forms, rank, world, port, cfg)


def _buffer_both_forms(rank, world, port, cfg):
    import deep_ep
    from oracle.bf16 import bits_to_torch, torch_to_bits
    mp_workers._set_device(rank)
    quant, i32, capture = cfg
    group = mp_workers._init(rank, world, port)
    E, K, H, T_max = 256, 8, 7168, 4096
    os.environ["DEEPEP_WINDOW_BYTES"] = str(6 * (T_max * K * H * 2 + (8 << 20)) + (4 << 20))     # combine slots: the largest region
    buf = deep_ep.Buffer(group, low_latency_mode=True)
    assert buf.runtime.get_dispatch_stage_local()          # on by default
    qk = {None: False, "int8": True, "pertoken_fp8_e4m3": "fp8"}[quant]

    def run(x, ti, tw, worst=0):
        per_rank, _, per_expert, is_in, _ = buf.get_dispatch_layout(ti, E)
        rx, _, _, lst, handle, _ = buf.dispatch(x, num_tokens_per_rank=per_rank, is_token_in_rank=is_in, num_tokens_per_expert=per_expert,
                                                topk_idx=ti, topk_weights=tw, quant_mode=quant, num_worst_tokens=worst)
        rx, rs = rx if quant else (rx, None)
        y = (rx.float() * rs[:, None]).to(torch.bfloat16) if quant else rx
        out, _, _ = buf.combine(y, handle)
        return [rx.view(torch.uint8) if quant else rx, rs, handle[3], out], lst

    # T = 300 first, then 4096 twice: the second call receives far more rows than the speculative guess (exact-size retry), the third hits
    for it, T in enumerate((300, T_max, T_max)):
        xs, idxs, ws = mp_workers.make_inputs(1, T, H, K, E, 0.1, seed=500 + it)
        xs, idxs, ws = [xs[0][:T]], [idxs[0][:T]], [np.abs(ws[0][:T])]
        idxs[0][7, :] = -1                                   # a token that selects nothing
        x = bits_to_torch(xs[0]).cuda()
        ti = torch.from_numpy(idxs[0].astype(np.int32) if i32 else idxs[0]).cuda()
        tw = torch.from_numpy(ws[0]).cuda()
        res = {}
        for on in (False, True, False, True):                # each form twice, alternating: the speculative guess is shared
            buf.runtime.set_dispatch_stage_local(on)
            buf.begin_profile(0, 1, "")
            got, lst = run(x, ti, tw)
            buf.end_profile()
            names = {k for k, (n, _) in buf.get_profile_summary().items() if n}
            assert ("dispatch_stage_local" in names) == on and ("dispatch_stage" in names) == (not on), names
            if on in res:
                assert all(torch.equal(a, b) for a, b in zip(res[on][0], got) if a is not None)
            res[on] = (got, lst)
        (a, la), (b, lb) = res[False], res[True]
        assert la == lb
        for u, v in zip(a, b):
            if u is not None:
                assert torch.equal(u, v)
        want = O.normal_dispatch(xs, [idxs[0]], E, qk)[0]
        n = want.total_recv
        assert lb == want.num_recv_tokens_per_expert_list
        gx = b[0].cpu().numpy()[:n] if quant else torch_to_bits(b[0])[:n]
        assert np.array_equal(gx, want.recv_x[:n].view(gx.dtype))
        if quant:
            assert np.array_equal(b[1].cpu().numpy()[:n].view(np.uint32), want.recv_x_scales[:n].view(np.uint32))
        assert np.array_equal(b[2].cpu().numpy()[:3 * n], want.recv_src_idx[:3 * n])
        ys = [O.per_token_cast_back(want.recv_x, want.recv_x_scales) if quant else want.recv_x]
        comb = O.combine(ys, [want.recv_src_idx], [n], [idxs[0]], ws, E)[0]
        assert np.array_equal(torch_to_bits(b[3]), comb)
        # num_worst_tokens (no host sync): worst-case sized outputs, same rows and combine
        worst = T * K
        wres = {}
        for on in (False, True):
            buf.runtime.set_dispatch_stage_local(on)
            wres[on], lw = run(x, ti, tw, worst)
            assert lw == [] and wres[on][0].shape[0] == worst
        (ux, us, ui, uo), (vx, vs, vi, vo) = wres[False], wres[True]      # rows past the received total are never written
        assert torch.equal(ux[:n], vx[:n]) and torch.equal(ui[:3 * n], vi[:3 * n]) and torch.equal(uo, vo)
        assert us is None or torch.equal(us[:n], vs[:n])
        assert torch.equal(vx[:n], b[0][:n]) and torch.equal(vo, b[3])
    if capture:
        # the num_worst_tokens pair captured in a graph (the two-launch form is captured the same way in test_deep_ep_gpu) and replayed
        T = 512
        x_s = torch.zeros((T, H), dtype=torch.bfloat16, device="cuda")
        ti_s = torch.zeros((T, K), dtype=torch.int32 if i32 else torch.int64, device="cuda")
        tw_s = torch.zeros((T, K), dtype=torch.float32, device="cuda")

        def load(seed):
            xs, idxs, ws = mp_workers.make_inputs(1, T, H, K, E, 0.1, seed=seed)
            x_s.copy_(bits_to_torch(xs[0][:T]).cuda())
            ti_s.copy_(torch.from_numpy(idxs[0][:T]).cuda())
            tw_s.copy_(torch.from_numpy(np.abs(ws[0][:T])).cuda())

        buf.runtime.set_dispatch_stage_local(True)
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
            load(200 + rep)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for on in (True, False):
                buf.runtime.set_dispatch_stage_local(on)
                eager, _ = run(x_s, ti_s, tw_s, T * K)
                torch.cuda.synchronize()
                n = int((ti_s >= 0).sum().item())
                assert torch.equal(cap[0][:n], eager[0][:n]) and torch.equal(cap[2][:3 * n], eager[2][:3 * n]), (rep, on)
                if quant:
                    assert torch.equal(cap[1][:n], eager[1][:n]), (rep, on)
                assert torch.equal(cap[3], eager[3]), (rep, on)
            buf.runtime.set_dispatch_stage_local(True)
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("cfg", [(None, False, False), ("int8", False, True), ("int8", True, False), ("pertoken_fp8_e4m3", True, True)],
                         ids=["bf16", "int8_graph", "int8_i32idx", "fp8_i32idx_graph"])
def test_buffer_dispatch_combine_with_and_without_stage_local(cfg):
    _spawn(_buffer_worker, 1, cfg)
