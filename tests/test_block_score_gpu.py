"""GPU parity of the block-score indexer (C-ABI mi_gqa_block_score_topk / mi_topk_append_local_block, torch.ops.npu.gqa_block_score_topk and
sgl_kernel_npu.indexer.flash_block_score_decode) against the stored outputs of the reference kernel and against the float64 restatement
(tests/block_score_ref.py), at the tolerant top-k criterion with TOL = 8 x the measured fp32 error (block_score_ref.py's header).

Every case of the table keeps NaN in the K rows behind a sequence's end inside its last block and in a page no sequence owns, and every
table entry of a block at or behind the end names that page: a read through such an entry, or of such a row, shows as a wrong row, never
as a fault.  Every C-ABI run keeps sentinels behind the output and the workspace."""
import glob
import os
from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import block_score_ref as R
from capi import load, ptr, stream_ptr
from sparse_decode_ref import sparse_decode_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = sorted(glob.glob(os.path.join(GOLD, "block_score_ref_fp16_*.npz")))
EINVAL = -1
DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1}
DTYPES = [torch.bfloat16, torch.float16]
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load("libmi_sgl_kernels.so")
        _lib.mi_gqa_block_score_topk_workspace.restype = c_size_t
        _lib.mi_gqa_block_score_topk_workspace.argtypes = [c_int] * 3
        _lib.mi_gqa_block_score_topk.argtypes = (
            [c_void_p] * 4 + [c_int]                            # q k topk_idx seq_lens | packed
            + [c_void_p, c_int, c_int64, c_int64, c_int]        # block_table, is_i64, strides, columns
            + [c_void_p, c_int, c_int64, c_int64, c_int]        # req_to_token, is_i64, strides, columns
            + [c_void_p, c_int]                                 # req_pool_indices
            + [c_int] * 13                                      # batch q_heads kv_heads head_dim block_size max_seqblock topk init local lse append pages sanitize
            + [c_int64] * 5 + [c_float, c_int, c_void_p, c_size_t, c_void_p])
        _lib.mi_topk_append_local_block.argtypes = [c_void_p] * 3 + [c_int] * 5 + [c_void_p]
    return _lib


def is64(t):
    return int(t.dtype == torch.int64)


def to_gpu(c):
    """A case of block_score_ref.make_case / load_golden on the GPU (the K cache keeps its strides: it is cut from its base buffer there)."""
    g = dict(c)
    for key, val in c.items():
        if isinstance(val, torch.Tensor) and key not in ("k", "k_base"):
            g[key] = val.cuda()
    if "k_base" in c:
        g["k_base"] = c["k_base"].cuda()
        g["k"] = g["k_base"][..., :c["k"].shape[-1]]
        assert g["k"].stride() == c["k"].stride()
    else:
        g["k"] = c["k"].cuda()
    return g


def run_capi(c, fused=False, expect=0, **over):
    """-> (topk_idx [Hq, B, topk (+ 1)], fp32 scores [B, Hq, max_seqblock]); `over` replaces integer arguments of the call."""
    L = lib()
    q, k = c["q"], c["k"]
    B, Hq, D = q.shape
    bs, Hkv = k.shape[1], k.shape[2]
    a = dict(batch=B, q_heads=Hq, kv_heads=Hkv, head_dim=D, block_size=bs, max_seqblock=-(-c["max_seqlen"] // bs), topk=c["topk"],
             init=c["init_blocks"], local=c["local_blocks"], lse=int(c["score_type"] == "lse"), append=c["max_num_blocks"] if fused else 0,
             num_pages=c.get("num_pages", 1), sanitize=int(c.get("sanitize", False)), sm_scale=c["sm_scale"], ws_short=0)
    a.update(over)
    direct = "req_to_token" in c
    tab = c["req_to_token"] if direct else c["block_table"]
    lens = c["seq_lens"].to(torch.int32)
    width = a["topk"] + (1 if fused else 0)
    wsb = L.mi_gqa_block_score_topk_workspace(B, Hq, max(a["max_seqblock"], 1) if a["max_seqblock"] <= 16384 else 1)
    tail = 256
    ws = torch.full((wsb + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    n_out = Hq * B * max(width, 0)
    flat = torch.full((n_out + tail,), -77, dtype=torch.int32, device="cuda")
    pool = c["req_pool_indices"] if direct else None
    rc = L.mi_gqa_block_score_topk(
        ptr(q), ptr(k), ptr(flat), ptr(lens), int(c.get("packed", False)),
        None if direct else ptr(tab), is64(tab), tab.stride(0), tab.stride(1), 0 if direct else tab.shape[1],
        ptr(tab) if direct else None, is64(tab), tab.stride(0), tab.stride(1), tab.shape[1] if direct else 0,
        ptr(pool), is64(pool) if direct else 0,
        a["batch"], a["q_heads"], a["kv_heads"], a["head_dim"], a["block_size"], a["max_seqblock"], a["topk"], a["init"], a["local"], a["lse"],
        a["append"], a["num_pages"], a["sanitize"], q.stride(0), q.stride(1), k.stride(0), k.stride(1), k.stride(2), a["sm_scale"],
        DTYPE_CODE[q.dtype], ptr(ws), wsb - a["ws_short"], stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((flat[n_out:] == -77).all()), "wrote behind the output"
    assert bool((ws[wsb:] == 0xA5).all()), "wrote behind the workspace"
    if expect:
        assert bool((flat == -77).all()), "a refused call wrote"
        return None, None
    scores = ws[:wsb].view(torch.float32).view(B, Hq, -1)
    return flat[:n_out].view(Hq, B, width), scores


def run_python(c, fused=False, sync=True, **extra):
    from sgl_kernel_npu.indexer.flash_block_score_decode import flash_decode_bnsd_with_topk_idx
    kw = dict(c.get("knobs", {}))
    kw.update(extra)
    if "req_to_token" in c:
        kw.update(req_to_token=c["req_to_token"], req_pool_indices=c["req_pool_indices"], num_pages=c["num_pages"],
                  sanitize_page_ids=c.get("sanitize", False))
    if "req_to_token" in c or fused:
        kw.update(max_num_blocks=c["max_num_blocks"])
    o, idx = flash_decode_bnsd_with_topk_idx(c["q"], None, c["k"], None, c.get("block_table"), c["seq_lens"], c["max_seqlen"], c["block_size"],
                                             c["topk"], c["init_blocks"], c["local_blocks"], c["sm_scale"], c["score_type"],
                                             disable_index_value=True, packed_seq_lens=c.get("packed", False), fused_append_local=fused, **kw)
    assert o is None and idx.dtype == torch.int32
    if sync:
        torch.cuda.synchronize()
    return idx


def restate(c, fused=False):
    return R.block_topk_ref(c["q"], c["k"], c["seq_lens"], c["block_size"], c["max_seqlen"], c["topk"], c["init_blocks"], c["local_blocks"],
                            fused_append_local=fused, max_num_blocks=c["max_num_blocks"], **R.ref_kwargs(c))


def check_scores(gpu_scores, scores, scored):
    """The workspace keeps the natural scores of the rows that were scored: each within TOL of its float64 value."""
    gpu_scores = gpu_scores.cpu().double().numpy()
    worst = 0.0
    for b, rows in enumerate(scores):
        for h, nat in enumerate(rows):
            if scored[b][h] and len(nat):
                worst = max(worst, float(np.abs(gpu_scores[b, h, :len(nat)] - nat).max()))
    print("max |score_gpu - score_f64|", worst, "TOL", R.TOL)
    assert worst <= R.TOL, worst


def check_case(c, got, want, scores, scored, fused=False):
    topk = c["topk"]
    assert tuple(got.shape) == want.shape, (got.shape, want.shape)
    got = got.cpu()
    R.check_all(got, scores, scored, topk, c["init_blocks"], c["local_blocks"])
    if fused:                                                   # slot topk follows from the entries in front of it
        G = got.shape[0] // c["k"].shape[2]
        again = R.append_rows_ref(got[:, :, :topk], c["seq_lens"].cpu(), c["block_size"], c["max_num_blocks"], c.get("packed", False), G)
        assert np.array_equal(got.numpy(), again), "the appended slot / the entry check"


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
@pytest.mark.parametrize("entry", ["capi", "python"])
def test_against_reference_kernel_outputs(path, entry):
    c = R.load_golden(path)
    g = to_gpu(c)
    got = run_capi(g, c["fused"])[0] if entry == "capi" else run_python(g, c["fused"])
    print(os.path.basename(path), entry, got[:, 0].tolist())
    R.check_golden(got.cpu(), c)


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_against_restatement(case, dtype):
    c = R.make_case(*case, dtype)
    g = to_gpu(c)
    want, scores, scored = restate(c)
    got, gpu_scores = run_capi(g)
    check_scores(gpu_scores, scores, scored)
    check_case(c, got, want, scores, scored)
    check_case(c, run_python(g), want, scores, scored)
    for other in ("max", "lse"):                                # the other score type on the same inputs (C-ABI)
        if other != c["score_type"]:
            c2, g2 = dict(c, score_type=other), dict(g, score_type=other)
            want2, scores2, scored2 = restate(c2)
            got2, gpu_scores2 = run_capi(g2)
            check_scores(gpu_scores2, scores2, scored2)
            check_case(c2, got2, want2, scores2, scored2)


@pytest.mark.parametrize("name", ["mha_bs16", "g4_bs64_lse", "packed_direct", "forced_gt_nb"])
def test_masked_keys_and_unused_table_entries_do_not_matter(name):
    """The case with NaN behind every sequence's end and in the page no sequence owns, against the same case with those rows zeroed and the
    unused table entries naming page 0: identical rows and, where scored, bit-identical finite scores."""
    case = next(c for c in R.CASES if c[0] == name)
    c = R.make_case(*case, torch.float16)
    assert bool(torch.isnan(c["k_base"]).any())
    clean = dict(c, k_base=torch.nan_to_num(c["k_base"], nan=0.0))
    clean["k"] = clean["k_base"][..., :c["k"].shape[-1]]
    poison = c["k"].shape[0] - 1
    if "block_table" in c:
        assert bool((c["block_table"] == poison).any())
        clean["block_table"] = torch.where(c["block_table"] == poison, 0, c["block_table"])
    else:
        assert bool((c["req_to_token"] == poison * c["block_size"]).any())
        clean["req_to_token"] = torch.where(c["req_to_token"] == poison * c["block_size"], 0, c["req_to_token"])
    a, sa = run_capi(to_gpu(c))
    b, sb = run_capi(to_gpu(clean))
    assert torch.equal(a, b)
    _, scores, scored = restate(c)
    for bi, rows in enumerate(scores):
        for h, nat in enumerate(rows):
            if scored[bi][h] and len(nat):
                row = sa[bi, h, :len(nat)]
                assert bool(torch.isfinite(row).all()) and torch.equal(row, sb[bi, h, :len(nat)])


def check_attention(got, want, exact, dtype):
    """test_gqa_sparse_decode_gpu.check."""
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


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,Hq,Hkv,D,bs,lens,topk", [(3, 16, 2, 128, 64, [640, 333, 1], 12), (2, 8, 1, 64, 16, [100, 160], 10),
                                                      (2, 16, 4, 128, 128, [1024, 700], 8)])
def test_pipeline_with_every_block_selected_equals_decode_gqa(B, Hq, Hkv, D, bs, lens, topk, dtype):
    """score -> normalise -> sparse decode with topk >= nb for every row: every block once, -1 behind them, so the result is paged GQA
    decode.  A repeated block in a padding slot (what the reference writes there) would be attended twice and show here."""
    from sgl_kernel_npu.attention.decode_attention import decode_gqa
    from sgl_kernel_npu.attention.gqa_share_sparse_attention import flash_decode_bnsd_with_gqa_share_sparse
    from sgl_kernel_npu.indexer.flash_block_score_decode import _normalize_topk_idx_for_gqa
    c = to_gpu(R.attention_case(B, Hq, Hkv, D, bs, lens, dtype, seed=11, topk=topk))
    assert all(-(-n // bs) <= topk for n in lens)
    idx = run_python(c)
    assert idx.shape == (Hq, B, topk) and bool((idx == -1).any())
    lists = _normalize_topk_idx_for_gqa(idx, Hq, Hkv, Hq // Hkv)
    assert lists.shape == (Hkv, B, topk)
    got = flash_decode_bnsd_with_gqa_share_sparse(c["q"], None, c["k"], c["v"], c["block_table"], c["seq_lens"], bs, lists, c["sm_scale"])
    dense = torch.empty_like(c["q"])
    decode_gqa(c["q"], c["k"], c["v"], dense, c["seq_lens"], c["sm_scale"], bs, c["block_table"])
    torch.cuda.synchronize()
    exact = torch.from_numpy(sparse_decode_ref(c["q"], c["k"], c["v"], lists, c["seq_lens"], bs, block_table=c["block_table"], sm_scale=c["sm_scale"]))
    check_attention(got, dense.cpu(), exact, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("score_type", ["max", "lse"])
def test_full_form_returns_dense_attention_and_the_list(dtype, score_type):
    from sgl_kernel_npu.indexer.flash_block_score_decode import flash_decode_bnsd_with_topk_idx
    c = to_gpu(R.full_form_case(dtype, score_type))
    (B, Hq, D), Hkv, bs, topk = c["q"].shape, c["k"].shape[2], c["block_size"], c["topk"]
    o, idx = flash_decode_bnsd_with_topk_idx(c["q"], c["sink"], c["k"], c["v"], c["block_table"], c["seq_lens"], c["max_seqlen"], bs, topk, 1, 1,
                                             c["sm_scale"], score_type, num_kv_chunks=2)
    torch.cuda.synchronize()
    want, scores, scored = restate(c)
    check_case(c, idx, want, scores, scored)
    mb = c["block_table"].shape[1]
    every = torch.arange(mb).expand(Hkv, B, mb)
    kw = dict(block_table=c["block_table"], sink=c["sink"], sm_scale=c["sm_scale"])
    exact = torch.from_numpy(sparse_decode_ref(c["q"], c["k"], c["v"], every, c["seq_lens"], bs, **kw))
    ref = exact if dtype == torch.float16 else torch.from_numpy(sparse_decode_ref(c["q"], c["k"], c["v"], every, c["seq_lens"], bs, round_p=dtype, **kw)).to(dtype)
    check_attention(o, ref, exact, dtype)


@pytest.mark.parametrize("name", ["g4_bs64_lse", "mha_bs16", "packed_direct", "g4_max_nofor"])
def test_append_fused_and_standalone_agree(name):
    from sgl_kernel_npu.indexer.flash_block_score_decode import append_local_block_to_topk_idx
    case = next(c for c in R.CASES if c[0] == name)
    c = R.make_case(*case, torch.float16)
    g = to_gpu(c)
    want, scores, scored = restate(c, fused=True)
    for entry in ("capi", "python"):
        fused = run_capi(g, fused=True)[0] if entry == "capi" else run_python(g, fused=True)
        check_case(c, fused, want, scores, scored, fused=True)
        if not c["packed"]:                                     # the standalone op takes one length per sequence
            plain = run_python(g)
            two = append_local_block_to_topk_idx(plain, g["seq_lens"], c["block_size"], c["max_num_blocks"])
            torch.cuda.synchronize()
            assert torch.equal(two, fused), entry


def test_append_standalone_against_restatement():
    """Entries of every kind: holes, blocks behind the end and behind num_blocks, the local block present / absent, an empty sequence."""
    L = lib()
    g = torch.Generator().manual_seed(3)
    H, B, topk, bs, nblk = 3, 5, 70, 16, 12
    lens = torch.tensor([0, 1, 100, 192, 500], dtype=torch.int32)
    idx = torch.randint(-2, 16, (H, B, topk), generator=g).to(torch.int32)
    idx[0, :, :] = torch.randint(-1, 3, (B, topk), generator=g).to(torch.int32)      # rows that mostly miss the local block
    want = R.append_local_ref(idx, lens, bs, nblk)
    from sgl_kernel_npu.indexer.flash_block_score_decode import append_local_block_to_topk_idx
    for lt in (torch.int32, torch.int64):
        got = append_local_block_to_topk_idx(idx.cuda(), lens.to(lt).cuda(), bs, nblk)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
    flat = torch.full((H * B * (topk + 1) + 64,), -77, dtype=torch.int32, device="cuda")
    di, dl = idx.cuda(), lens.cuda()
    assert L.mi_topk_append_local_block(ptr(di), ptr(dl), ptr(flat), H, B, topk, bs, nblk, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(flat[:H * B * (topk + 1)].view(H, B, topk + 1).cpu().numpy(), want) and bool((flat[H * B * (topk + 1):] == -77).all())
    assert L.mi_topk_append_local_block(ptr(di), ptr(dl), ptr(flat), H, B, topk, 0, nblk, stream_ptr()) == EINVAL
    assert L.mi_topk_append_local_block(ptr(di), ptr(dl), ptr(flat), H, B, topk, bs, 0, stream_ptr()) == EINVAL
    assert L.mi_topk_append_local_block(ptr(di), ptr(dl), None, H, B, topk, bs, nblk, stream_ptr()) == EINVAL


def test_captured_in_a_graph_follows_new_lengths_table_and_q():
    """Nothing is read back on the host: captured once (one stream, no branches), replayed after lengths, table and q changed in place."""
    problems = R.graph_cases()
    c = to_gpu(problems[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_python(c, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run_python(c, fused=True, sync=False)
    for p in problems:
        for key in ("seq_lens", "block_table", "q"):
            c[key].copy_(p[key])
        out.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        fresh = run_python(c, fused=True)
        assert torch.equal(replayed, fresh), p["seq_lens"]
        want, scores, scored = restate(p, fused=True)
        check_case(p, replayed, want, scores, scored, fused=True)


def test_at_the_declared_limits():
    c = R.limits_case()
    want, scores, scored = restate(c)
    got, gpu_scores = run_capi(to_gpu(c))
    check_scores(gpu_scores, scores, scored)
    check_case(c, got, want, scores, scored)
    check_case(c, run_python(to_gpu(c)), want, scores, scored)


def test_argument_checks_and_limits_raise():
    from sgl_kernel_npu.indexer.flash_block_score_decode import flash_decode_bnsd_with_topk_idx as f
    case = next(c for c in R.CASES if c[0] == "g4_bs64_lse")
    c = to_gpu(R.make_case(*case, torch.float16))
    d = to_gpu(R.make_case(*next(x for x in R.CASES if x[0] == "g32_direct"), torch.float16))
    L = lib()
    assert L.mi_gqa_block_score_topk_workspace(2, 8, 100) == 2 * 8 * 100 * 4
    assert L.mi_gqa_block_score_topk_workspace(2, 8, 16384) == 2 * 8 * 16384 * 4 and L.mi_gqa_block_score_topk_workspace(2, 8, 16385) == 0
    run_capi(c)                                                                                 # the case itself is served
    for over in (dict(max_seqblock=16385), dict(max_seqblock=0), dict(topk=1025), dict(topk=0), dict(block_size=48), dict(head_dim=60),
                 dict(head_dim=264), dict(sm_scale=0.0), dict(kv_heads=3), dict(init=-1), dict(local=-1), dict(ws_short=4)):
        run_capi(c, expect=EINVAL, **over)
    run_capi(dict(c, req_to_token=d["req_to_token"], req_pool_indices=d["req_pool_indices"]), expect=EINVAL, num_pages=0)
    q, k, bt, lens = c["q"], c["k"], c["block_table"], c["seq_lens"]
    so = dict(disable_index_value=True)
    with pytest.raises(AssertionError):
        f(q, None, k, None, bt, lens, 64 * 16384 + 1, 64, 8, 0, 0, **so)                        # more than 16384 blocks
    with pytest.raises(AssertionError):
        f(q, None, k, None, bt, lens, 3000, 64, 1025, 0, 0, **so)
    with pytest.raises(RuntimeError):
        torch.ops.npu.gqa_block_score_topk(q, k, bt, lens, 64 * 16384 + 1, 8, 0, 0, 0.1)
    with pytest.raises(RuntimeError):
        torch.ops.npu.gqa_block_score_topk(q, k, bt, lens, 3000, 1025, 0, 0, 0.1)
    with pytest.raises(RuntimeError):
        torch.ops.npu.gqa_block_score_topk(q, k[:, :, :, :60], bt, lens, 3000, 8, 0, 0, 0.1)    # head dims differ
    with pytest.raises(RuntimeError):
        torch.ops.npu.gqa_block_score_topk(q, k, bt, lens, 3000, 8, 0, 0, 0.1, append_local=True)      # no max_num_blocks
    # the tuning knobs of the reference are accepted and change nothing
    base = f(q, None, k, None, bt, lens, c["max_seqlen"], 64, 8, 2, 2, score_type="lse", **so)[1]
    knobs = f(q, None, k, None, bt, lens, c["max_seqlen"], 64, 8, 2, 2, score_type="lse", num_kv_chunks=4, max_num_kv_chunks=2, use_triton_topk=True,
              num_topk_chunks=4, use_chunked_score=False, score_blocks_per_chunk=2, score_max_chunks=4, runtime_fill_only=True,
              runtime_score_short_max_blocks=8, runtime_score_short_chunks=2, use_native=False, **so)[1]
    assert torch.equal(base, knobs)
    o, empty = f(q, None, k, None, bt, lens, c["max_seqlen"], 64, 0, 0, 0, **so)
    assert o is None and empty.shape == (8, 6, 0) and empty.is_cuda
