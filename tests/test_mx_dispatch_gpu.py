"""Normal dispatch in the OCP MX block-scaled modes (MXFP8 E4M3 / E5M2, MXFP4 E2M1) on the MI355X.  Through the C-ABI: every staging and
receive entry point (stage + pull, stage_compact + pull_indexed / pull_local, stage_push + pull_indexed, stage_local) against
tests/mx_ref.py, rows with the contract's edge blocks included, and the H % 32 rejection.  Through deep_ep.Buffer (W = 1, 2, 4
processes): both transports, stage_local, the alltoall strategy, long-sequence rounds, num_worst_tokens, the tuple input, and
combine of the de-quantised rows."""
import ctypes

import numpy as np
import pytest
import torch

import ep_harness as Hh
import mp_workers
import mx_ref as M
import mx_workers
from capi import ptr, ptr_array, stream_ptr
from test_deep_ep_plumbing_cpu import _spawn as _spawn_ranks

pytestmark = pytest.mark.gpu


def _lib():
    lib = Hh.lib()
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.mi_ep_dispatch_stage_local.argtypes = [V, V, I, V, V, V, I, I, I, I, I, I, V, V, V, V, V]
    lib.mi_ep_dispatch_stage_local.restype = ctypes.c_int
    return lib


def _inputs(T, H, K, E, seed):
    xs, idxs, _ = mp_workers.make_inputs(1, T, H, K, E, 0.1, seed=seed)
    idx = idxs[0]
    if T > 1:
        idx[1, :] = -1                                    # a token that selects nothing
    return mx_workers.with_edge_rows(xs, H)[0], idx


def _check(got_x, got_s, got_tri, want, mode, H):
    r, d, s, fin = want
    n = r.total_recv
    assert np.array_equal(got_tri.cpu().numpy()[:3 * n], r.recv_src_idx[:3 * n])
    gs = got_s.cpu().numpy()[:n * (H // 32)].reshape(n, H // 32)
    assert np.array_equal(gs, s), (mode, H, np.argwhere(gs != s)[:4])
    gx = got_x.cpu().numpy()[:n]
    mask = np.repeat(fin, 16 if mode == "mx_fp4_e2m1" else 32, axis=1)
    assert np.array_equal(gx[mask], d[mask]), (mode, H, np.argwhere((gx != d) & mask)[:4])
    # the receive buffers past the rows written keep their sentinels
    assert (got_x.cpu().numpy()[n:] == 0x5A).all() and (got_s.cpu().numpy()[n * (H // 32):] == 0x5A).all()


@pytest.mark.parametrize("H", [7168, 2048, 32])
@pytest.mark.parametrize("mode", M.MODES)
def test_c_abi_every_transport_at_one_rank(mode, H):
    lib = _lib()
    qm = M.QM[mode]
    T, K, E = 48, 4, 16
    x_bits, idx = _inputs(T, H, K, E, seed=H)
    want = M.mx_dispatch([x_bits], [idx], E, mode)[0]
    R = want[0].total_recv
    x = torch.from_numpy(x_bits.view(np.int16)).cuda()
    ti = torch.from_numpy(idx).cuda()
    lay = Hh.layout(ti, E, 1)
    cnt = lay["num_tokens_per_expert"]
    recv_count = torch.cumsum(cnt, 0, dtype=torch.int32)
    pull_offset = lay["send_data_offset"]            # W = 1: the exclusive prefix, also relative to the own (only) source
    rb = lib.mi_ep_dispatch_row_bytes(H, qm)
    data_b = H // 2 if mode == "mx_fp4_e2m1" else H
    assert rb == ((data_b + H // 32 + 16 + 127) // 128) * 128
    st = stream_ptr()
    # every launch form writes into fresh sentinel-filled buffers with two rows of slack
    rows = R + 2

    def bufs():
        return (torch.full((rows, data_b), 0x5A, dtype=torch.uint8, device="cuda"),
                torch.full((rows * (H // 32),), 0x5A, dtype=torch.uint8, device="cuda"),
                torch.full((rows * 3,), -9, dtype=torch.int32, device="cuda"))

    i32idx = int(ti.dtype == torch.int32)
    sm = lay["send_token_idx_small"]
    region = torch.zeros(T * (rb + 8 * K) + 4096, dtype=torch.uint8, device="cuda")
    forms = {}
    # replicated staging + pull (the alltoall strategy's kernels)
    rep = torch.zeros(T * K * rb, dtype=torch.uint8, device="cuda")
    Hh.ck(lib.mi_ep_dispatch_stage(ptr(x), ptr(ti), i32idx, ptr(sm), ptr(lay["send_data_offset"]), T, K, H, E, 0, qm, ptr(rep), st))
    rx, rs, tri = bufs()
    Hh.ck(lib.mi_ep_dispatch_pull(ptr_array([rep.data_ptr()]), ptr(recv_count), ptr(pull_offset), 1, E, H, qm, R, ptr(rx), ptr(rs),
                                  ptr(tri), st))
    forms["stage+pull"] = (rx, rs, tri)
    # compact staging + pull_indexed, and + pull_local
    Hh.ck(lib.mi_ep_dispatch_stage_compact(ptr(x), ptr(ti), i32idx, ptr(sm), ptr(lay["send_data_offset"]), T, K, H, E, 0, qm,
                                           ptr(region), region.numel(), None, 0, st))
    rx, rs, tri = bufs()
    Hh.ck(lib.mi_ep_dispatch_pull_indexed(ptr_array([region.data_ptr()]), ptr(recv_count), ptr(pull_offset), 1, E, H, K, qm, R,
                                          region.numel(), ptr(rx), ptr(rs), ptr(tri), None, 0, -1, st))
    forms["compact+pull_indexed"] = (rx, rs, tri)
    rx, rs, tri = bufs()
    Hh.ck(lib.mi_ep_dispatch_pull_local(ptr(region), ptr(ti), i32idx, ptr(sm), ptr(recv_count), ptr(cnt), T, K, H, E, 1, 0, qm, R,
                                        ptr(rx), ptr(rs), ptr(tri), None, None, 0, st))
    forms["compact+pull_local"] = (rx, rs, tri)
    # push staging (one source slab) + pull_indexed
    slab_region = torch.zeros(region.numel(), dtype=torch.uint8, device="cuda")
    Hh.ck(lib.mi_ep_dispatch_stage_push(ptr(x), ptr(ti), i32idx, ptr(sm), ptr(lay["send_data_offset"]), T, K, H, E, 1, 0, qm,
                                        ptr_array([slab_region.data_ptr()]), slab_region.numel(), None, 0, st))
    slab = lib.mi_ep_dispatch_push_slab_bytes(slab_region.numel(), 1)
    rx, rs, tri = bufs()
    Hh.ck(lib.mi_ep_dispatch_pull_indexed(ptr_array([slab_region.data_ptr()]), ptr(recv_count), ptr(pull_offset), 1, E, H, K, qm, R,
                                          slab, ptr(rx), ptr(rs), ptr(tri), None, 0, -1, st))
    forms["push+pull_indexed"] = (rx, rs, tri)
    # one launch at one rank
    rx, rs, tri = bufs()
    Hh.ck(lib.mi_ep_dispatch_stage_local(ptr(x), ptr(ti), i32idx, ptr(sm), ptr(recv_count), ptr(cnt), T, K, H, E, qm, R, ptr(rx),
                                         ptr(rs), ptr(tri), None, st))
    forms["stage_local"] = (rx, rs, tri)
    torch.cuda.synchronize()
    for name, (rx, rs, tri) in forms.items():
        try:
            _check(rx, rs, tri, want, mode, H)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


def test_c_abi_rejects_hidden_not_multiple_of_32():
    lib = _lib()
    T, K, E, H = 8, 2, 4, 48
    x = torch.zeros((T, H), dtype=torch.bfloat16, device="cuda")
    ti = torch.zeros((T, K), dtype=torch.int64, device="cuda")
    lay = Hh.layout(ti, E, 1)
    rows = torch.zeros(T * K * 256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(T * K * 256, dtype=torch.uint8, device="cuda")
    cnt = lay["num_tokens_per_expert"]
    st = stream_ptr()
    for qm in M.QM.values():
        assert lib.mi_ep_dispatch_stage(ptr(x), ptr(ti), 0, ptr(lay["send_token_idx_small"]), ptr(lay["send_data_offset"]), T, K, H,
                                        E, 0, qm, ptr(rows), st) == -1
        assert lib.mi_ep_dispatch_stage_local(ptr(x), ptr(ti), 0, ptr(lay["send_token_idx_small"]), ptr(cnt), ptr(cnt), T, K, H, E,
                                              qm, T * K, ptr(out), ptr(out), ptr(out), None, st) == -1
        assert lib.mi_ep_dispatch_pull(ptr_array([rows.data_ptr()]), ptr(cnt), ptr(cnt), 1, E, H, qm, T * K, ptr(out), ptr(out),
                                       ptr(out), st) == -1
    # the same H is fine without block scales
    assert lib.mi_ep_dispatch_stage(ptr(x), ptr(ti), 0, ptr(lay["send_token_idx_small"]), ptr(lay["send_data_offset"]), T, K, H, E,
                                    0, Hh.QUANT_INT8, ptr(rows), st) == 0
    torch.cuda.synchronize()


def _spawn(fn, world, cfg):
    procs = mp_workers.ranks_on_first_gpu(world) + 1
    if procs > mp_workers.MAX_PROCS_PER_GPU:
        pytest.skip(f"{world} ranks on one GPU make {procs} processes on it, at most {mp_workers.MAX_PROCS_PER_GPU} may share a GPU")
    _spawn_ranks(fn, world, cfg)


@pytest.mark.parametrize("cfg", [
    # W, T, H, K, E, drop, strategy, variant
    (1, 64, 7168, 8, 256, 0.1, "default", "transports"),      # stage_local and stage + pull_local
    (1, 40, 32, 4, 16, 0.1, "default", "transports"),         # a single block per row
    (2, 48, 2048, 4, 16, 0.2, "default", "transports"),       # push and pull
    (4, 33, 7168, 8, 256, 0.0, "default", "transports"),
    (4, 24, 32, 4, 16, 0.1, "default", "transports"),
    (2, 100, 2048, 4, 16, 0.1, "default", "rounds"),          # DEEPEP_NORMAL_LONG_SEQ_ROUND = 4 x 32 tokens
    (1, 64, 2048, 4, 16, 0.1, "alltoall", "transports"),
], ids=lambda c: "-".join(map(str, c)))
def test_mx_dispatch_through_buffer(cfg):
    _spawn(mx_workers.gpu_mx_worker, cfg[0], cfg)
