"""GPU: the sparse_attn_sharedkv kernel (csrc/kernels/sparse_sharedkv.hip) against the float64 restatement of tests/sparse_sharedkv_ref.py,
through the C-ABI and through torch.ops.npu.sparse_attn_sharedkv: the case table (every cache row no token may read holds NaN), ill-formed
index lists, explicit split counts, graph replay, lightning_indexer -> sparse_attn_sharedkv end to end, the stored outputs of the reference
test's golden, and the refusals.  Tolerance: atol 1e-3, rtol 2^-7 (bf16) / 2^-10 (fp16), the project's figures for an MFMA online-softmax
kernel against a P-rounded golden; the stored reference cases at the reference test's own 2e-2."""
from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import sparse_sharedkv_ref as R
from capi import load, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
SENTINEL = 0x5A


def _lib():
    lib = load("libmi_sgl_kernels.so")
    lib.mi_sparse_attn_sharedkv_workspace.restype = c_size_t
    lib.mi_sparse_attn_sharedkv_workspace.argtypes = [c_int64, c_int64, c_int]
    lib.mi_sparse_attn_sharedkv.restype = c_int
    lib.mi_sparse_attn_sharedkv.argtypes = ([c_void_p] * 11 + [c_int, c_int, c_int, c_int64] + [c_int] * 7 + [c_int64] * 12 +
                                            [c_float] + [c_int] * 5 + [c_void_p, c_size_t, c_void_p])
    return lib


def _op():
    import sgl_kernel_npu  # noqa: F401

    return torch.ops.npu.sparse_attn_sharedkv


def on_gpu(c):
    """The case's tensors on the GPU; the caches keep their strided page dimension."""
    g = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    g["ori_kv"] = R.paged_view(g["ori_base"], c["ori_block"])
    g["cmp_kv"] = R.paged_view(g["cmp_base"], c["cmp_block"]) if c.get("cmp_base") is not None else None
    assert g["ori_kv"].stride(0) == c["ori_block"] * R.D + R.PAD
    return g


def run_op(g, **over):
    kw = dict(ori_kv=g["ori_kv"], cmp_kv=g["cmp_kv"], cmp_sparse_indices=g.get("cmp_sparse_indices"), ori_block_table=g["ori_block_table"],
              cmp_block_table=g.get("cmp_block_table"), cu_seqlens_q=g.get("cu_seqlens_q"), seqused_q=g.get("seqused_q"),
              seqused_kv=g["seqused_kv"], sinks=g["sinks"], softmax_scale=g["softmax_scale"], cmp_ratio=g["cmp_ratio"],
              ori_win_left=g["ori_win_left"], ori_win_right=g["ori_win_right"], layout_q=g["layout_q"])
    kw.update(over)
    q = kw.pop("q", g["q"])
    return _op()(q, **kw)


def list_bound(g):
    win = min(g["ori_win_left"] + g["ori_win_right"] + 1, g["ori_block_table"].shape[1] * g["ori_block"])
    if g.get("cmp_sparse_indices") is not None:
        return win + g["cmp_sparse_indices"].shape[-1]
    return win + (g["cmp_block_table"].shape[1] * g["cmp_block"] if g["cmp_kv"] is not None else 0)


def run_capi(g, num_splits=0, expect=0, **over):
    """-> out (q's shape).  Sentinel bytes sit behind the output and behind the workspace and must survive; a refused call (expect != 0)
    must leave the output untouched as well."""
    lib = _lib()
    a = dict(g)
    a.update(over)
    q = a["q"]
    tnd = a["layout_q"] == "TND"
    tokens = q.shape[0] if tnd else q.shape[0] * q.shape[1]
    heads, dim = a.get("heads", q.shape[-2]), a.get("dim", q.shape[-1])
    cu = a.get("cu_seqlens_q")
    B = q.shape[0] if not tnd else cu.numel() - 1 if cu is not None else a["seqused_kv"].numel()
    S1 = 1 if tnd else q.shape[1]
    nbytes = q.numel() * 2
    obuf = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = obuf[:nbytes].view(q.dtype).view(q.shape)
    wsb = lib.mi_sparse_attn_sharedkv_workspace(tokens, list_bound(a), num_splits) if tokens else 0
    ws = torch.full((wsb + 256,), SENTINEL, dtype=torch.uint8, device=DEV)
    ix, cmp = a.get("cmp_sparse_indices"), a["cmp_kv"]
    cbt = a.get("cmp_block_table")
    K = a.get("K", ix.shape[-1] if ix is not None else 0)
    rc = lib.mi_sparse_attn_sharedkv(
        ptr(q), ptr(a["ori_kv"]), ptr(cmp), ptr(out), ptr(a["sinks"]), ptr(ix), ptr(a["ori_block_table"]), ptr(cbt), ptr(a.get("cu_seqlens_q")),
        ptr(a.get("seqused_q")), ptr(a["seqused_kv"]), 1 if tnd else 0, B, S1, tokens, heads, dim, a["ori_kv"].shape[1],
        a["ori_block_table"].shape[1], cmp.shape[1] if cmp is not None else 0, cbt.shape[1] if cbt is not None else 0, K,
        0 if tnd else q.stride(0), q.stride(0) if tnd else q.stride(1), q.stride(-2), 0 if tnd else out.stride(0),
        out.stride(0) if tnd else out.stride(1), out.stride(-2), ix.stride(0) if ix is not None and not tnd else 0,
        ix.stride(0 if tnd else 1) if ix is not None else 0, a["ori_kv"].stride(0), cmp.stride(0) if cmp is not None else 0,
        a["ori_block_table"].stride(0), cbt.stride(0) if cbt is not None else 0, a["softmax_scale"], a["cmp_ratio"], a["ori_win_left"],
        a["ori_win_right"], 0 if q.dtype == torch.bfloat16 else 1, num_splits, ptr(ws), wsb, stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((obuf[nbytes:] == SENTINEL).all()), "bytes behind the output were written"
    assert bool((ws[wsb:] == SENTINEL).all()), "bytes behind the workspace were written"
    if expect != 0:
        assert bool((obuf == SENTINEL).all()) and bool((ws == SENTINEL).all()), "a refused call wrote something"
    return out


def check(got, want, dtype, what):
    got = got.detach().cpu().double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the output (a poisoned row was read)"
    err = (got - want).abs()
    print(what, "max abs err", float(err.max()), "max err / (atol + rtol |want|)",
          float((err / (R.tol(dtype)["atol"] + R.tol(dtype)["rtol"] * want.abs())).max()))
    assert torch.allclose(got, want, **R.tol(dtype)), what


# ---- 1. the case table, through the C-ABI and through the op
@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,li", R.VARIANTS, ids=[f"{n}{li}" for n, li in R.VARIANTS])
def test_case_table(name, li, dtype):
    c, want = R.case(name, li, dtype)
    g = on_gpu(c)
    check(run_capi(g), want, dtype, f"{c['name']} C-ABI")
    out, lse = run_op(g, metadata=torch.zeros(1024, dtype=torch.int32, device=DEV))
    check(out, want, dtype, f"{c['name']} op")
    assert lse.dtype == torch.float32 and lse.numel() == 0 and out.shape == g["q"].shape and out.dtype == dtype


# ---- 2. ill-formed lists: every slot is judged on its own
def _ill_formed(c, r, limit, K, rng):
    row = np.full(K, -1, dtype=np.int64)
    if r % 4 == 3:
        return row                                              # an all-(-1) row
    vis = rng.permutation(max(limit, 1))[:K // 2] if limit else np.array([], dtype=np.int64)
    row[:len(vis)] = vis
    rng.shuffle(row)                                            # -1 in the middle
    row[0], row[1] = limit, limit + 7                           # entries >= limit
    row[2], row[3] = -5, -(2 ** 31)                             # other negatives
    if len(vis):
        row[4] = row[5] = vis[0]                                # duplicates (they count every time)
        row[K - 1] = vis[-1]                                    # a valid entry in the last slot, behind the -1s
    return row


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
def test_ill_formed_index_lists(dtype):
    c = R.make_case("ill", "TND", [1500, 640, 257, 3], [2, 3, 2, 1], 64, 16, "sparse", 4, (5, 0), "normal", K=96, dtype=dtype, seed=31,
                    index_rows=_ill_formed)
    idx = c["cmp_sparse_indices"].reshape(-1, 96)
    assert (idx[3] == -1).all() and idx[0, :4].tolist() == [374, 381, -5, -(2 ** 31)]      # row 0: p = 1498, limit = 374
    want = R.attend_ref(c)
    g = on_gpu(c)
    check(run_capi(g), want, dtype, "ill-formed C-ABI")
    check(run_op(g)[0], want, dtype, "ill-formed op")


# ---- 3. explicit split counts through the C-ABI
@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["c", "e"])
def test_explicit_splits(name, dtype):
    for li in (0, 2):
        c, want = R.case(name, li, dtype)
        g = on_gpu(c)
        for n in (1, 2, 5):
            check(run_capi(g, num_splits=n), want, dtype, f"{c['name']} splits {n}")
    # more pieces than the list has tiles: case c's decode rows hold 128 + 11 positions at most (three tiles)
    c, want = R.case("c", 0, dtype)
    assert max(int(n) for n in c["seqused_kv"]) // 128 + 128 <= 3 * 64
    check(run_capi(on_gpu(c), num_splits=7), want, dtype, "c0 splits 7 > tiles")


# ---- 4. graph replay: the launches are sized from host integers alone
def test_graph_replay_reads_the_current_inputs():
    dtype = torch.bfloat16
    cases = [R.case("e", 0, dtype, seed=s) for s in (None, 1, 2)]
    g = on_gpu(cases[0][0])
    keys = ("q", "seqused_kv", "ori_block_table", "cmp_block_table", "cmp_sparse_indices", "ori_base", "cmp_base", "sinks")
    for c, _ in cases[1:]:
        assert all(c[k].shape == cases[0][0][k].shape for k in keys)
    run_op(g)                                                   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        out, _ = run_op(g)
    torch.cuda.synchronize()
    for c, want in cases[1:]:
        for k in keys:
            g[k].copy_(c[k].to(DEV))                            # in place: the captured launches see the same storage
        graph.replay()
        torch.cuda.synchronize()
        check(out, want, dtype, f"replay with {c['name']} lengths {c['seqused_kv'].tolist()[:3]}..")


# ---- 5. lightning_indexer -> sparse_attn_sharedkv
def test_indexer_output_feeds_the_attention():
    import sgl_kernel_npu  # noqa: F401

    dtype, K = torch.bfloat16, 64
    c = R.make_case("e2e", "BSND", [640, 3, 257, 129, 1500], 1, 128, 16, "dense", 4, (127, 0), "normal", dtype=dtype, seed=77)
    g = on_gpu(c)
    B = len(c["seqused_kv"])
    gen = torch.Generator().manual_seed(5)
    iq = torch.randn(B, 1, 64, 128, generator=gen).to(dtype).to(DEV)
    iw = torch.rand(B, 1, 64, generator=gen).to(dtype).to(DEV)
    ikey = torch.randn(g["cmp_kv"].shape[0], 16, 1, 128, generator=gen).to(dtype).to(DEV)      # index keys in the pages of cmp_block_table
    visible = (c["seqused_kv"] // 4).to(torch.int32).to(DEV)                                 # limit of a decode row: L // cmp_ratio
    idx = torch.ops.npu.lightning_indexer(iq, ikey, iw, None, visible, g["cmp_block_table"], "BSND", "PA_BSND", K, 0)
    assert idx.shape == (B, 1, 1, K) and idx.dtype == torch.int32
    rows = idx.cpu().reshape(B, K)
    for b in range(B):
        n = min(K, int(visible[b]))
        assert (rows[b, :n] >= 0).all() and (rows[b, :n] < int(visible[b])).all() and (rows[b, n:] == -1).all()
    out, _ = run_op(g, cmp_sparse_indices=idx)
    want = R.attend_ref(c, indices=idx.cpu())                   # the same returned indices: selection ties play no part
    check(out, want, dtype, "indexer -> attention")


# ---- 6. the stored outputs of the reference test's golden
@pytest.mark.parametrize("path", R.golden_paths(), ids=lambda p: p.split("_")[-1][:1])
def test_stored_reference_cases(path):
    c = R.load_golden(path)
    g = on_gpu(c)
    heads = torch.from_numpy(c["golden_heads"]).long()
    for what, out in (("C-ABI", run_capi(g)), ("op", run_op(g)[0])):
        got = out.cpu().float()[:, :, heads]
        print(c["name"], what, "max abs err", float((got - c["golden"]).abs().max()))
        torch.testing.assert_close(got, c["golden"], rtol=2e-2, atol=2e-2)


# ---- 7. refusals
def test_refusals_launch_nothing_and_write_nothing():
    c, _ = R.case("e", 2, torch.bfloat16)
    g = on_gpu(c)
    run_capi(g, expect=EINVAL, heads=32)
    run_capi(g, expect=EINVAL, dim=256)
    run_capi(g, expect=EINVAL, cmp_ratio=3)
    run_capi(g, expect=EINVAL, K=4096)
    run_capi(g, expect=EINVAL, cu_seqlens_q=None, layout_q="TND", q=g["q"])          # TND without cu_seqlens_q
    run_capi(g, expect=EINVAL, cmp_kv=None)                                           # cmp_sparse_indices without cmp_kv
    run_capi(g, expect=EINVAL, cmp_block_table=None)                                  # cmp_kv without cmp_block_table
    run_capi(g, expect=EINVAL, num_splits=65)
    canary = g["q"].clone()
    bad = [
        (dict(q=g["q"][:, :32]), "64 query heads"),
        (dict(q=g["q"][:, :, :256], ori_kv=g["ori_kv"][..., :256]), "512"),
        (dict(cmp_kv=g["cmp_kv"].to(torch.float16)), "cmp_kv dtype must match q dtype"),
        (dict(cmp_ratio=3), "cmp_ratio"),
        (dict(ori_mask_mode=3), "ori_mask_mode"),
        (dict(return_softmax_lse=True), "return_softmax_lse"),
        (dict(ori_sparse_indices=g["cmp_sparse_indices"]), "ori_sparse_indices"),
        (dict(layout_kv="BSND"), "PA_ND"),
        (dict(cu_seqlens_q=None), "cu_seqlens_q is required"),
        (dict(cmp_kv=None), "cmp_kv is required when cmp_sparse_indices is present"),
        (dict(cmp_block_table=None), "cmp_block_table is required when cmp_kv is present"),
        (dict(cmp_sparse_indices=torch.zeros(g["q"].shape[0], 1, 4096, dtype=torch.int32, device=DEV)), "2048"),
        (dict(metadata=torch.zeros(8, dtype=torch.int32, device=DEV)), "metadata"),
    ]
    for over, text in bad:
        with pytest.raises(RuntimeError, match=text):
            run_op(g, **over)
    torch.cuda.synchronize()
    assert torch.equal(canary, g["q"])
    # B = 0 / T = 0: an empty result, no launch
    out, lse = run_op(g, q=g["q"][:0], cu_seqlens_q=torch.zeros(1, dtype=torch.int32, device=DEV), seqused_kv=g["seqused_kv"][:0],
                      ori_block_table=g["ori_block_table"][:0], cmp_block_table=g["cmp_block_table"][:0],
                      cmp_sparse_indices=g["cmp_sparse_indices"][:0])
    assert out.shape == (0, 64, 512) and lse.numel() == 0
    c1, _ = R.case("a", 0, torch.bfloat16)
    g1 = on_gpu(c1)
    out, _ = run_op(g1, q=g1["q"][:0], seqused_kv=g1["seqused_kv"][:0], ori_block_table=g1["ori_block_table"][:0])
    assert out.shape == (0, 1, 64, 512)
    assert run_capi(g1, q=g1["q"][:0]).numel() == 0
