"""GPU parity of the block-sparse GQA decode (C-ABI mi_gqa_sparse_decode, torch.ops.npu.gqa_share_sparse_decode and
sgl_kernel_npu.attention.gqa_share_sparse_attention.flash_decode_bnsd_with_gqa_share_sparse) against the stored outputs of the reference
Triton kernel and against the float64 restatement (tests/sparse_decode_ref.py), at the criterion of test_gqa_gpu.check.

Every C-ABI run here keeps sentinels behind the output and the workspace, and every table entry that must not be used -- blocks at or behind
a sequence's end, columns behind the table's extent -- names a page of NaNs that lies inside the cache allocation but behind the pages the
case uses: a read through such an entry shows as a wrong value, never as a fault."""
import glob
import os
from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from capi import load, ptr, stream_ptr
from sparse_decode_ref import sparse_decode_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = sorted(glob.glob(os.path.join(GOLD, "gqa_sparse_ref_fp16_*.npz")))
EINVAL, ENOTAPPLICABLE = -1, -3
DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load("libmi_sgl_kernels.so")
        _lib.mi_gqa_sparse_decode_workspace.restype = c_size_t
        _lib.mi_gqa_sparse_decode_workspace.argtypes = [c_int] * 4
        _lib.mi_gqa_sparse_decode_num_chunks.argtypes = [c_int] * 3
        _lib.mi_gqa_sparse_decode.argtypes = (
            [c_void_p] * 6 + [c_int] + [c_int64] * 3            # q k v out seq_lens topk_idx | is_i64, three strides
            + [c_void_p, c_int, c_int64, c_int64]               # block_table
            + [c_void_p, c_int, c_int64, c_int64, c_int]        # req_to_token, cols
            + [c_void_p, c_int]                                 # req_pool_indices
            + [c_void_p, c_int, c_int64]                        # sink, dtype, row stride
            + [c_int] * 9                                       # batch q_heads kv_heads head_dim block_size topk max_kv_len num_pages sanitize
            + [c_int64] * 10 + [c_float, c_int, c_int, c_void_p, c_size_t, c_void_p])
    return _lib


def is64(t):
    return int(t.dtype == torch.int64)


def run_capi(c, num_chunks, expect=0):
    """c: dict of GPU tensors q k v topk_idx seq_lens (int32) + block_table | (req_to_token, req_pool_indices, max_num_blocks, num_pages,
    sanitize) + optional sink, sm_scale.  Returns the output; asserts the sentinels behind output and workspace."""
    L = lib()
    q, k, v, idx = c["q"], c["k"], c["v"], c["topk_idx"]
    B, Hq, D = q.shape
    bs, Hkv, topk = k.shape[1], k.shape[2], idx.shape[2]
    direct = "req_to_token" in c
    tab = c["req_to_token"] if direct else c["block_table"]
    max_kv_len = (c["max_num_blocks"] if direct else tab.shape[1]) * bs
    sink = c.get("sink")
    nc = num_chunks
    if not nc:                                                 # the library's choice: a power of two within the list
        nc = L.mi_gqa_sparse_decode_num_chunks(B, Hkv, topk)
        assert nc >= 1 and nc & (nc - 1) == 0 and nc <= max(1, topk), nc
    wsb = L.mi_gqa_sparse_decode_workspace(B, Hq, D, nc)
    assert (wsb == 0) == (nc == 1)
    tail = 256
    ws = torch.full((wsb + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    flat = torch.full((B * Hq * D + tail,), -77.0, dtype=q.dtype, device="cuda")
    out = flat[:B * Hq * D].view(B, Hq, D)
    idx_sh = idx.stride(0) * (1 if idx.shape[0] == Hkv else Hq // Hkv)
    rc = L.mi_gqa_sparse_decode(
        ptr(q), ptr(k), ptr(v), ptr(out), ptr(c["seq_lens"]), ptr(idx), is64(idx), idx_sh, idx.stride(1), idx.stride(2),
        None if direct else ptr(tab), is64(tab), tab.stride(0), tab.stride(1),
        ptr(tab) if direct else None, is64(tab), tab.stride(0), tab.stride(1), tab.shape[1] if direct else 0,
        ptr(c["req_pool_indices"]) if direct else None, is64(c["req_pool_indices"]) if direct else 0,
        ptr(sink), DTYPE_CODE[sink.dtype] if sink is not None else 0, sink.stride(0) if sink is not None else 0,
        B, Hq, Hkv, D, bs, topk, max_kv_len, c.get("num_pages", 1), int(c.get("sanitize", False)),
        q.stride(0), q.stride(1), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1),
        c["sm_scale"], DTYPE_CODE[q.dtype], num_chunks, ptr(ws), wsb, stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((flat[B * Hq * D:] == -77.0).all()), "wrote behind the output"
    assert bool((ws[wsb:] == 0xA5).all()), "wrote behind the workspace"
    return out


def run_python(c, num_topk_chunks, **extra):
    from sgl_kernel_npu.attention.gqa_share_sparse_attention import flash_decode_bnsd_with_gqa_share_sparse
    kw = dict(extra)
    if "req_to_token" in c:
        kw.update(req_to_token=c["req_to_token"], req_pool_indices=c["req_pool_indices"], max_num_blocks=c["max_num_blocks"],
                  num_pages=c["num_pages"], sanitize_page_ids=c.get("sanitize", False))
    out = flash_decode_bnsd_with_gqa_share_sparse(c["q"], c.get("sink"), c["k"], c["v"], c.get("block_table"), c["seq_lens"], c["k"].shape[1],
                                                  c["topk_idx"], c["sm_scale"], num_topk_chunks=num_topk_chunks, **kw)
    torch.cuda.synchronize()
    return out


def restate(c, round_p=None):
    kw = dict(sink=c.get("sink"), sm_scale=c["sm_scale"], round_p=round_p)
    if "req_to_token" in c:
        kw.update(req_to_token=c["req_to_token"], req_pool_indices=c["req_pool_indices"], max_num_blocks=c["max_num_blocks"],
                  num_pages=c["num_pages"], sanitize_page_ids=c.get("sanitize", False))
    else:
        kw.update(block_table=c["block_table"])
    return torch.from_numpy(sparse_decode_ref(c["q"], c["k"], c["v"], c["topk_idx"], c["seq_lens"], c["k"].shape[1], **kw))


def check(got, want, exact, dtype):
    """test_gqa_gpu.check: fp16 against `want` at atol = 1e-3, rtol = 2**-10; bf16: P is rounded to 8 bits before P.V in kernel and `want`
    alike, against different running maxima, so both are measured against the exact float64 result."""
    got = got.cpu()
    print("max abs error", (got.double() - exact).abs().max().item(), "of the comparison value", (want.double() - exact).abs().max().item())
    assert not torch.isnan(got.float()).any()
    if dtype == torch.float16:
        assert torch.allclose(got.float(), want.float(), atol=1e-3, rtol=2 ** -10), (got.float() - want.float()).abs().max()
        return
    err_k = (got.double() - exact).abs().max().item()
    err_o = (want.double() - exact).abs().max().item()
    assert err_k <= 1.5 * err_o + 1e-3, (err_k, err_o)
    assert torch.allclose(got.float(), want.float(), rtol=1e-2, atol=1e-2)


def chunk_counts(topk):
    return [n for n in (0, 1, 2, 4) if n <= max(1, topk)]


def golden_case(path):
    z = np.load(path)
    t = lambda key: torch.from_numpy(z[key]).cuda()
    c = dict(q=t("q"), k=t("k"), v=t("v"), topk_idx=t("topk_idx"), seq_lens=t("seq_lens"), sm_scale=float(z["sm_scale"]))
    if "sink" in z:
        c["sink"] = t("sink")
    if "block_table" in z:
        c["block_table"] = t("block_table")
    else:
        c.update(req_to_token=t("req_to_token"), req_pool_indices=t("req_pool_indices"), max_num_blocks=int(z["max_num_blocks"]),
                 num_pages=int(z["num_pages"]), sanitize=bool(z["sanitize_page_ids"]))
    return c, torch.from_numpy(z["out"])


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
@pytest.mark.parametrize("entry", ["capi", "python"])
def test_against_reference_kernel_outputs(path, entry):
    c, want = golden_case(path)
    for chunks in (1, 2, 4, None):
        got = run_capi(c, chunks or 0) if entry == "capi" else run_python(c, chunks)
        err = (got.cpu().float() - want.float()).abs().max().item()
        print(os.path.basename(path), entry, "chunks", chunks, "max abs error", err)
        assert torch.allclose(got.cpu().float(), want.float(), atol=1e-3, rtol=2 ** -10), (chunks, err)


def make_case(B, Hq, Hkv, D, bs, topk, lens, dtype, seed, max_blocks=None, idx_dtype=torch.int32, tab_dtype=torch.int32, direct=False,
              sanitize=False, sink=None, per_q=False, dup=False, one_buffer=False, full=False):
    """A sparse decode problem on the GPU.  Lists: a random subset of the logical blocks 0 .. max_blocks + 1 (so: some at or behind the
    sequence's end and some behind the table's extent) in random slots, holes elsewhere; the block holding the sequence's last key is in the
    list with probability 3/4, anywhere.  full = every block of the table once, in order (topk = max_blocks)."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lens, dtype=torch.int32)
    if max_blocks is None:
        max_blocks = (int(lens.max()) + bs - 1) // bs
    G = Hq // Hkv
    num_pages = B * max_blocks + 1
    poison = num_pages                                         # inside the allocation, behind the pages the case uses
    width = 2 * D if one_buffer else D
    buf = torch.randn((num_pages + 1, bs, Hkv, width), generator=g).to(dtype)
    buf[poison] = float("nan")
    buf = buf.cuda()
    if one_buffer:                                             # K and V are views of one buffer: rows 2 D apart
        k, v = buf[:num_pages, :, :, :D], buf[:num_pages, :, :, D:]
    else:
        k = buf[:num_pages]
        v2 = torch.randn((num_pages + 1, bs, Hkv, D), generator=g).to(dtype)
        v2[poison] = float("nan")
        v = v2.cuda()[:num_pages]
    q = torch.randn((B, Hq, D), generator=g).to(dtype).cuda()
    pages = torch.randperm(num_pages, generator=g)[:B * max_blocks].reshape(B, max_blocks)
    extent = max_blocks * bs
    heads = Hq if per_q else Hkv
    idx = torch.full((heads, B, topk), -1, dtype=torch.int64)
    for h in range(heads):
        for b in range(B):
            if full:
                idx[h, b] = torch.arange(topk)
                continue
            cand = torch.randperm(max_blocks + 2, generator=g)[:max(1, (2 * topk) // 3)].tolist()
            last = (min(int(lens[b]), extent) - 1) // bs
            if int(torch.randint(0, 4, (1,), generator=g)) and last not in cand:
                cand[0] = last
            slots = torch.randperm(topk, generator=g)[:len(cand)].tolist()
            for s, blk in zip(slots, cand):
                idx[h, b, s] = blk
            if dup and topk >= 2:
                src = slots[0]
                idx[h, b, (src + 1) % topk] = idx[h, b, src]
    c = dict(q=q, k=k, v=v, topk_idx=idx.to(idx_dtype).cuda(), seq_lens=lens.cuda(), sm_scale=float(D) ** -0.5)
    used = lambda b, j: j * bs < min(int(lens[b]), extent)
    if direct:
        rows, cols = B + 2, extent + 5
        rtt = torch.full((rows, cols), poison * bs, dtype=torch.int64)
        pool = torch.tensor([rows - 1 - b for b in range(B)], dtype=torch.int64)
        for b in range(B):
            for j in range(max_blocks):
                if used(b, j):
                    rtt[pool[b], j * bs:(j + 1) * bs] = pages[b, j] * bs + torch.arange(bs)
        c.update(req_to_token=rtt.to(tab_dtype).cuda(), req_pool_indices=pool.to(idx_dtype).cuda(), max_num_blocks=max_blocks,
                 num_pages=num_pages + 1, sanitize=sanitize)
    else:
        wide = torch.full((B, max_blocks + 8), poison, dtype=torch.int64)      # the table is a view: columns behind its extent name the NaN page
        for b in range(B):
            for j in range(max_blocks):
                if used(b, j):
                    wide[b, j] = pages[b, j]
        c["block_table"] = wide.to(tab_dtype).cuda()[:, :max_blocks]
    if sink is not None:
        c["sink"] = (torch.randn((Hq, D), generator=g) * 1.5).to(sink).cuda()
    return c


#  B  Hq  Hkv  D   bs  topk  lens               options
CASES = [
    (3, 16, 1, 128, 128, 17, [2000, 1, 1280], dict(sink="same")),                                  # a single key; exactly a block boundary
    (2, 64, 8, 128, 64, 32, [1500, 777], dict(idx_dtype=torch.int64, tab_dtype=torch.int64)),
    (2, 8, 8, 64, 16, 6, [150, 37], dict(sink=torch.float32, direct=True, one_buffer=True)),      # MHA; K and V views of one buffer
    (2, 128, 1, 256, 32, 9, [300, 256], dict(sink="same")),                                        # two head blocks per wave, 256-wide rows
    (2, 40, 1, 80, 64, 5, [333, 64], dict(direct=True, sanitize=True, per_q=True, tab_dtype=torch.int64)),   # padded head dim and head block
    (2, 16, 2, 64, 16, 64, [1024, 500], dict(max_blocks=40, dup=True, sink="same")),              # seq_lens above the table's extent; duplicates
    (1, 16, 1, 128, 32, 1, [70], dict()),                                                          # one slot
    (2, 8, 8, 256, 128, 3, [129, 384], dict(one_buffer=True, idx_dtype=torch.int64)),
    (1, 192, 1, 64, 16, 3, [40], dict(sink="same")),                                               # group > 128: two workgroups per unit
]


@pytest.mark.parametrize("B,Hq,Hkv,D,bs,topk,lens,opt", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_against_restatement(B, Hq, Hkv, D, bs, topk, lens, opt, dtype):
    opt = dict(opt)
    if opt.get("sink") == "same":
        opt["sink"] = dtype
    c = make_case(B, Hq, Hkv, D, bs, topk, lens, dtype, seed=B * 1000 + Hq + topk, **opt)
    exact = restate(c)
    want = exact if dtype == torch.float16 else restate(c, round_p=torch.bfloat16).to(torch.bfloat16)
    for chunks in chunk_counts(topk):
        print("chunks", chunks)
        check(run_capi(c, chunks), want, exact, dtype)
    check(run_python(c, None), want, exact, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Hq,Hkv,D,bs,lens", [(3, 64, 8, 128, 64, [640, 333, 1]), (2, 16, 1, 128, 128, [1024, 900]), (2, 8, 2, 64, 16, [100, 160])])
def test_full_list_without_sink_equals_decode_gqa(B, Hq, Hkv, D, bs, lens, dtype):
    """With every block of the table in the list, in order, the op is paged GQA decode: decode_gqa on the same caches, same criterion."""
    from sgl_kernel_npu.attention.decode_attention import decode_gqa
    max_blocks = (max(lens) + bs - 1) // bs
    c = make_case(B, Hq, Hkv, D, bs, max_blocks, lens, dtype, seed=7, full=True)
    bt = c["block_table"].clamp(max=c["k"].shape[0] - 1).contiguous()      # decode_gqa never reads behind a sequence's end; keep its table tidy anyway
    dense = torch.empty_like(c["q"])
    decode_gqa(c["q"], c["k"], c["v"], dense, c["seq_lens"], c["sm_scale"], bs, bt)
    torch.cuda.synchronize()
    exact = restate(c)
    for chunks in chunk_counts(max_blocks):
        check(run_capi(c, chunks), dense.cpu(), exact, dtype)


def test_unused_entries_are_never_dereferenced():
    """Every slot that is -1, names a block at or behind the sequence's end, or a column behind the table's extent leads -- if followed --
    to the page of NaNs, and the block table's own padding to it as well: outputs are finite and right, with lists that hold MOSTLY such
    entries; direct-map form too (without the clamp, which would hide the page id)."""
    for direct in (False, True):
        c = make_case(4, 16, 2, 64, 16, 24, [33, 16, 1, 200], torch.float16, seed=21, max_blocks=16, direct=direct)
        idx = c["topk_idx"].cpu()
        lens = c["seq_lens"].cpu()
        unused = (idx < 0) | (idx * 16 >= lens[None, :, None])
        assert unused.float().mean() > 0.5 and bool((idx >= 16).any())
        exact = restate(c)
        for chunks in chunk_counts(24):
            got = run_capi(c, chunks).cpu()
            assert torch.isfinite(got.float()).all()
            check(got, exact, exact, torch.float16)


def test_rows_without_a_key_are_zero_with_and_without_a_sink():
    for sink in (None, torch.float16):
        c = make_case(2, 8, 2, 64, 32, 4, [100, 50], torch.float16, seed=3, sink=sink)
        c["topk_idx"][0, 1] = -1                               # kv head 0 of sequence 1: nothing selected
        c["topk_idx"][1, 0] = torch.tensor([-1, 9, -1, 4], dtype=torch.int32, device="cuda")      # only blocks behind the end
        c["topk_idx"][0, 0] = torch.tensor([1, -1, 0, -1], dtype=torch.int32, device="cuda")
        for chunks in chunk_counts(4):
            got = run_capi(c, chunks).cpu()
            assert bool((got[1, 0:4] == 0).all()) and bool((got[0, 4:8] == 0).all()), chunks
            assert bool((got[0, 0:4] != 0).any())
            check(got, restate(c), restate(c), torch.float16)


def test_captured_in_a_graph_follows_new_lists_and_lengths():
    """Nothing is read back on the host: the op is captured once and replayed with other topk_idx / seq_lens contents."""
    dtype = torch.float16
    c = make_case(3, 16, 2, 128, 64, 8, [500, 300, 64], dtype, seed=5, max_blocks=8, sink=dtype)
    others = [make_case(3, 16, 2, 128, 64, 8, lens, dtype, seed=s, max_blocks=8, sink=dtype) for s, lens in ((6, [100, 512, 1]), (8, [333, 129, 400]))]
    for chunks in (1, 2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run_python(c, chunks)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run_python_nosync(c, chunks)
        for o in [c] + others:                                 # the captured contents, then two other problems of the same shape
            for key in ("q", "k", "v", "topk_idx", "seq_lens", "block_table", "sink"):
                c[key].copy_(o[key])
            out.fill_(9.0)
            graph.replay()
            torch.cuda.synchronize()
            check(out, restate(c), restate(c), dtype)


def run_python_nosync(c, chunks):
    from sgl_kernel_npu.attention.gqa_share_sparse_attention import flash_decode_bnsd_with_gqa_share_sparse
    return flash_decode_bnsd_with_gqa_share_sparse(c["q"], c.get("sink"), c["k"], c["v"], c["block_table"], c["seq_lens"], c["k"].shape[1],
                                                   c["topk_idx"], c["sm_scale"], num_topk_chunks=chunks)


def test_argument_checks_raise():
    from sgl_kernel_npu.attention.gqa_share_sparse_attention import flash_decode_bnsd_with_gqa_share_sparse as f
    c = make_case(2, 8, 2, 64, 16, 6, [90, 40], torch.float16, seed=1)
    d = make_case(2, 8, 2, 64, 16, 6, [90, 40], torch.float16, seed=1, direct=True)
    q, k, v, bt, lens, idx = c["q"], c["k"], c["v"], c["block_table"], c["seq_lens"], c["topk_idx"]
    direct = dict(req_to_token=d["req_to_token"], req_pool_indices=d["req_pool_indices"], max_num_blocks=d["max_num_blocks"], num_pages=d["num_pages"])
    bad = [
        lambda: f(q.float(), None, k, v, bt, lens, 16, idx),                                   # dtype
        lambda: f(q, None, k.to(torch.bfloat16), v, bt, lens, 16, idx),
        lambda: f(q, None, k, v[:, :8], bt, lens, 16, idx),                                    # cache shapes differ
        lambda: f(q, None, k, v, None, lens, 16, idx),                                         # no page source
        lambda: f(q, None, k, v, bt, lens, 16, idx, **direct),                                 # two page sources
        lambda: f(q, None, k, v, None, lens, 16, idx, req_to_token=d["req_to_token"]),         # half a direct map
        lambda: f(q, None, k, v, None, lens, 16, idx, **dict(direct, num_pages=None)),
        lambda: f(q, None, k, v, bt.float(), lens, 16, idx),
        lambda: f(q, None, k, v, bt, lens, 32, idx),                                           # block size of the cache
        lambda: f(q, None, k, v, bt, lens[:1], 16, idx),
        lambda: f(q, None, k, v, bt, lens, 16, idx, num_topk_chunks=3),                        # not a power of two
        lambda: f(q, None, k, v, bt, lens, 16, idx, num_topk_chunks=8),                        # more chunks than slots
        lambda: f(q, None, k, v, bt, lens, 16, idx, num_topk_chunks=0),
        lambda: f(q, None, k, v, bt, lens, 16, idx, topk_blocks_per_step=3),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(AssertionError):
            call()
            pytest.fail(f"call {i} did not raise")
    # the tuning knobs of the reference are accepted and change nothing
    base = f(q, None, k, v, bt, lens, 16, idx, num_topk_chunks=2)
    knobs = f(q, None, k, v, bt, lens, 16, idx, num_topk_chunks=2, topk_blocks_per_step=2, prefetch_idx=True, num_warps=8, num_stages=1, use_native=False)
    assert torch.equal(base, knobs)
    bounded = f(q, None, k, v, bt, lens, 16, idx, max_num_topk_chunks=1)
    assert torch.allclose(bounded.float(), base.float(), atol=1e-3, rtol=2 ** -10)
    # the C-ABI refuses what it does not serve, before any launch
    L = lib()
    assert L.mi_gqa_sparse_decode_workspace(2, 8, 64, 1) == 0 and L.mi_gqa_sparse_decode_workspace(2, 8, 80, 4) == 2 * 8 * 4 * 130 * 4
    assert L.mi_gqa_sparse_decode_workspace(2, 8, 264, 4) == 0
    for B, Hkv, topk in ((4, 1, 17), (128, 1, 17), (64, 8, 32), (1, 1, 1), (1, 1, 3), (1, 1, 4096)):
        n = L.mi_gqa_sparse_decode_num_chunks(B, Hkv, topk)
        assert 1 <= n <= max(1, topk) and n & (n - 1) == 0
    run_capi(c, 3)                                                                               # any count up to topk is served by the C-ABI
    run_capi(c, 7, expect=EINVAL)                                                                # more chunks than slots
    run_capi(dict(c, sm_scale=0.0), 1, expect=EINVAL)
    wide = dict(c, topk_idx=torch.full((2, 2, 4096), -1, dtype=torch.int32, device="cuda"))
    run_capi(wide, 1, expect=ENOTAPPLICABLE)                                                     # 4096 slots in one chunk
    assert bool((run_capi(wide, 4) == 0).all())
    with pytest.raises(RuntimeError):
        torch.ops.npu.gqa_share_sparse_decode(q, None, k[:, :, :, :60], v[:, :, :, :60], bt, lens, idx, 0.125, 1)      # head dims differ
