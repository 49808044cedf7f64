"""Multi-process workers of the MX dispatch tests (tests/test_mx_dispatch_gpu.py): deep_ep.Buffer dispatch in the three MX quant modes
against tests/mx_ref.py, then combine of the de-quantised rows against oracle.ep.combine."""
import os

import numpy as np
import torch
import torch.distributed as dist

import mx_ref as M
from mp_workers import _init, _set_device, make_inputs, run_guarded

TAG = {"mx_fp8_e4m3": torch.float8_e4m3fn, "mx_fp8_e5m2": torch.float8_e5m2, "mx_fp4_e2m1": torch.float4_e2m1fn_x2}

# edge values of the MX contract, one per block: zeros, bf16 subnormals only, subnormals next to a normal, maxima at 2^emax * 1.99 of
# every format (saturation), 2^-120, 2^127, Inf, -Inf, NaN
_EDGE = ["zero", "sub", "submix", 2.0 ** 2 * 1.99, 2.0 ** 8 * 1.99, 2.0 ** 15 * 1.99, 2.0 ** -120, 2.0 ** 127, np.inf, -np.inf, np.nan]


def _edge_block(kind, rng):
    sub = np.ldexp(rng.integers(1, 128, 32).astype(np.float64), -133) * rng.choice([-1.0, 1.0], 32)
    if isinstance(kind, str):
        if kind == "zero":
            return np.where(rng.random(32) < 0.5, -0.0, 0.0)
        if kind == "sub":
            return sub
        out = sub.copy()
        out[int(rng.integers(32))] = -1.5
        return out
    out = rng.standard_normal(32) * (kind if np.isfinite(kind) else 1.0) / 4
    out[int(rng.integers(32))] = kind
    return out


def with_edge_rows(xs, H, seed=5):
    """The first rows of every rank's x carry the edge blocks (block b of row t: kind (t + b) mod len(_EDGE)); the rest stays random."""
    from oracle.bf16 import f32_to_bf16_bits_rne
    rng = np.random.default_rng(seed)
    out = []
    for x in xs:
        x = x.copy()
        for t in range(min(len(x), len(_EDGE))):
            row = M.bf16_bits_to_f64(x[t]).copy()
            for b in range(H // 32):
                row[b * 32:(b + 1) * 32] = _edge_block(_EDGE[(t + b) % len(_EDGE)], rng)
            x[t] = f32_to_bf16_bits_rne(row.astype(np.float32))
        out.append(x)
    return out


def dequant_bits(data, scales, finite, mode):
    """bf16 bits of the de-quantised rows; blocks with unspecified elements (Inf / NaN in x) as zeros, so combine sums stay finite."""
    y = M.dequant_mx_rows(data, scales, mode)
    y = np.where(np.repeat(finite, 32, axis=1), y, 0.0).astype(np.float32)
    return M.bf16_round(y)


def same_bf16(a, b):
    """Bit equality of bf16 rows, every NaN pattern counting as NaN (the 2^127 edge blocks overflow in the combine sums, and the
    payload of an Inf - Inf NaN is the adder's choice)."""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    na, nb = (a & 0x7FFF) > 0x7F80, (b & 0x7FFF) > 0x7F80
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~na])


def check_mx_dispatch(rx, rs, handle, lst, want, mode, H, rank, check_send_head=True):
    """recv_x / scale bytes / triples / counts of one rank against the oracle; the returned rows are those a consumer de-quantises."""
    r, d, s, fin = want[rank]
    n = r.total_recv
    fp4 = mode == "mx_fp4_e2m1"
    assert rx.dtype == TAG[mode] and rx.shape[1] == (H // 2 if fp4 else H), (rx.dtype, tuple(rx.shape))
    assert rs.dtype == torch.float8_e8m0fnu and rs.dim() == 1 and rs.numel() == rx.shape[0] * (H // 32), (rs.dtype, tuple(rs.shape))
    assert lst == r.num_recv_tokens_per_expert_list, (lst, r.num_recv_tokens_per_expert_list)
    assert np.array_equal(handle[3].cpu().numpy()[:3 * n], r.recv_src_idx[:3 * n])
    if check_send_head:
        assert np.array_equal(handle[5].cpu().numpy(), r.send_head)
    gx = rx.view(torch.uint8).cpu().numpy()[:n]
    gs = rs.view(torch.uint8).cpu().numpy()[:n * (H // 32)].reshape(n, H // 32)
    assert np.array_equal(gs, s), (mode, np.argwhere(gs != s)[:4])
    # element bytes: every block whose elements the contract specifies (the neighbours of an Inf / NaN block included)
    per = 16 if fp4 else 32
    mask = np.repeat(fin, per, axis=1)
    assert np.array_equal(gx[mask], d[mask]), (mode, np.argwhere((gx != d) & mask)[:4])
    return n


def gpu_mx_worker(rank, world, port, cfg):
    run_guarded(_gpu_mx, rank, world, port, cfg)


def _gpu_mx(rank, world, port, cfg):
    import deep_ep
    from oracle import ep as O
    from oracle.bf16 import bits_to_torch, torch_to_bits
    _set_device(rank)
    W, T, H, K, E, drop, strategy, variant = cfg
    assert W == world
    if variant == "rounds":
        os.environ["DEEPEP_NORMAL_LONG_SEQ_ROUND"] = str(-(-T // 32))
        os.environ["DEEPEP_NORMAL_LONG_SEQ_PER_ROUND_TOKENS"] = "32"
    group = _init(rank, world, port, "nccl" if strategy == "alltoall" else "gloo")
    os.environ.setdefault("DEEPEP_WINDOW_BYTES", str(768 << 20))
    os.environ.setdefault("DEEPEP_TIMEOUT_MS", "20000")
    buf = deep_ep.Buffer(group, low_latency_mode=True, normal_strategy=strategy, low_latency_strategy=strategy)
    assert buf.normal_strategy.get_name() == strategy
    xs, idxs, ws = make_inputs(W, T, H, K, E, drop, seed=77)
    xs = with_edge_rows(xs, H)
    x = bits_to_torch(xs[rank]).cuda()
    ti = torch.from_numpy(idxs[rank]).cuda()
    tw = torch.from_numpy(ws[rank]).cuda()
    per_rank, _, per_expert, is_in, _ = buf.get_dispatch_layout(ti, E)
    # the forms of the default strategy: both transports at W > 1; at W = 1 the one-launch stage_local and stage + pull_local
    forms = [None]
    if strategy == "default" and variant == "transports":
        forms = ["push", "pull"] if W > 1 else [True, False]
    for mode in M.MODES:
        want = M.mx_dispatch(xs, idxs, E, mode)
        ys = [dequant_bits(d, s, fin, mode) for (_, d, s, fin) in want]
        comb_want = O.combine(ys, [w[0].recv_src_idx for w in want], [w[0].total_recv for w in want], idxs, ws, E)
        for i, form in enumerate(forms):
            if isinstance(form, str):
                buf.runtime.set_dispatch_transport(form)
            elif isinstance(form, bool):
                buf.runtime.set_dispatch_stage_local(form)
            # the reference's tuple input (x, tag) for one form of every mode, quant_mode names otherwise
            tuple_form = i == len(forms) - 1
            arg = (x, torch.empty(0, dtype=TAG[mode], device="cuda")) if tuple_form else x
            (rx, rs), _, _, lst, handle, _ = buf.dispatch(arg, num_tokens_per_rank=per_rank, is_token_in_rank=is_in,
                                                          num_tokens_per_expert=per_expert, topk_idx=ti, topk_weights=tw,
                                                          quant_mode=None if tuple_form else mode)
            check_mx_dispatch(rx, rs, handle, lst, want, mode, H, rank, check_send_head=strategy == "default")
            out, _, _ = buf.combine(bits_to_torch(ys[rank]).cuda(), handle)
            assert same_bf16(torch_to_bits(out), comb_want[rank]), (mode, form, "combine mismatch")
            if strategy == "default" and variant == "transports" and i == 0:
                # DeepEP's graph-friendly mode: worst-case sized outputs, no host sync, empty count list
                worst = (T + W) * K * W                    # >= every rank's received rows (rank r holds T + r tokens)
                (rxw, rsw), _, _, lst_w, handle_w, _ = buf.dispatch(x, num_tokens_per_rank=per_rank, is_token_in_rank=is_in,
                                                                    num_tokens_per_expert=per_expert, topk_idx=ti, topk_weights=tw,
                                                                    quant_mode=mode, num_worst_tokens=worst)
                assert lst_w == [] and rxw.shape[0] == worst and rsw.numel() == worst * (H // 32)
                r0 = want[rank][0]
                saved = r0.num_recv_tokens_per_expert_list
                r0.num_recv_tokens_per_expert_list = []
                try:
                    check_mx_dispatch(rxw, rsw, handle_w, lst_w, want, mode, H, rank, check_send_head=False)
                finally:
                    r0.num_recv_tokens_per_expert_list = saved
                out_w, _, _ = buf.combine(bits_to_torch(ys[rank]).cuda(), handle_w)
                assert same_bf16(torch_to_bits(out_w), comb_want[rank]), (mode, "combine after worst-token dispatch mismatch")
    # hidden sizes that are no multiple of 32: a clear error naming the mode and H (every rank raises before any exchange)
    if variant == "transports" and H % 32 == 0:
        xh = x[:, :H - 16].contiguous()
        for mode in M.MODES:
            try:
                buf.dispatch(xh, num_tokens_per_rank=per_rank, is_token_in_rank=is_in, num_tokens_per_expert=per_expert,
                             topk_idx=ti, topk_weights=tw, quant_mode=mode)
                raise AssertionError(f"{mode} with hidden {H - 16} must be rejected")
            except (RuntimeError, ValueError) as e:
                assert mode in str(e) and str(H - 16) in str(e) and "32" in str(e), str(e)
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
