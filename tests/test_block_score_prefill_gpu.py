"""GPU parity of the prefill block-score indexer (C-ABI mi_gqa_prefill_block_score / mi_prefill_topk_from_score, torch.ops.npu.
gqa_prefill_block_score / prefill_topk_from_score and sgl_kernel_npu.indexer.flash_block_score_prefill) against the stored outputs of the
reference kernels and against the float64 restatement (tests/block_score_prefill_ref.py), at block_score_ref.TOL.

Every case of the table keeps NaN in the K rows behind a request's end inside its last block and in a page no request owns, and every
req_to_token entry of a block at or behind the end names that page: a read through such an entry, or of such a row, shows as a wrong
score, never as a fault.  Every C-ABI run writes into a NaN-filled score buffer with sentinels behind it."""
import glob
import os
from ctypes import c_float, c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

import block_score_prefill_ref as P
from capi import load, ptr, stream_ptr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1}
DTYPES = [torch.bfloat16, torch.float16]
_lib = None
_ref = {}


def lib():
    global _lib
    if _lib is None:
        _lib = load("libmi_sgl_kernels.so")
        _lib.mi_gqa_prefill_block_score.argtypes = (
            [c_void_p] * 3 + [c_void_p, c_int] * 2              # q k score | cu_seqlens, seq_lens (+ is_i64)
            + [c_void_p, c_int, c_int64, c_int64, c_int]        # req_to_token, is_i64, strides, columns
            + [c_void_p, c_int] * 2                             # req_pool_indices, query_pos (+ is_i64)
            + [c_int] * 8                                       # total_q num_reqs idx_heads kv_heads head_dim block_size max_seqblock lse
            + [c_int64] * 7 + [c_float, c_int, c_void_p])
        _lib.mi_prefill_topk_from_score.argtypes = [c_void_p] + [c_int64] * 3 + [c_void_p, c_int, c_void_p] + [c_int] * 6 + [c_void_p]
    return _lib


def is64(t):
    return int(t is not None and t.dtype == torch.int64)


def golden(letter):
    return P.load_golden(os.path.join(GOLD, f"block_score_prefill_ref_fp16_{letter}.npz"))


def to_gpu(c):
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


def restated(key, c, score_type=None, query_pos=None):
    """The float64 restatement, computed once per session for each (input, score type, convention)."""
    k = (key, score_type or c["score_type"], query_pos is not None)
    if k not in _ref:
        _ref[k] = P.restate(c, query_pos=query_pos, score_type=score_type)
    return _ref[k]


def run_capi_score(g, score_type=None, query_pos=None, expect=0, **over):
    """-> score [H, total_q, max_seqblock] written by the C-ABI into a NaN-filled buffer; `over` replaces integer arguments."""
    L = lib()
    q, k = g["q"], g["k"]
    total_q, H, D = q.shape
    bs, Hkv = k.shape[1], k.shape[2]
    a = dict(total_q=total_q, num_reqs=g["seq_lens"].shape[0], heads=H, kv_heads=Hkv, head_dim=D, block_size=bs,
             max_seqblock=-(-g["max_seqlen"] // bs), lse=int((score_type or g["score_type"]) == "lse"), sm_scale=g["sm_scale"])
    a.update(over)
    msb = max(a["max_seqblock"], 1) if a["max_seqblock"] <= 16384 else 1
    n_out, tail = H * total_q * msb, 256
    flat = torch.full((n_out + tail,), float("nan"), dtype=torch.float32, device="cuda")
    rtt, qp = g["req_to_token"], query_pos
    rc = L.mi_gqa_prefill_block_score(
        ptr(q), ptr(k), ptr(flat), ptr(g["cu_seqlens"]), is64(g["cu_seqlens"]), ptr(g["seq_lens"]), is64(g["seq_lens"]), ptr(rtt), is64(rtt),
        rtt.stride(0), rtt.stride(1), rtt.shape[1], ptr(g["req_pool_indices"]), is64(g["req_pool_indices"]), ptr(qp) if qp is not None else None,
        is64(qp), a["total_q"], a["num_reqs"], a["heads"], a["kv_heads"], a["head_dim"], a["block_size"], a["max_seqblock"], a["lse"],
        q.stride(0), q.stride(1), k.stride(0), k.stride(1), k.stride(2), total_q * msb, msb, a["sm_scale"], DTYPE_CODE[q.dtype], stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool(torch.isnan(flat[n_out:]).all()), "wrote behind the output"
    if expect:
        assert bool(torch.isnan(flat).all()), "a refused call wrote"
        return None
    score = flat[:n_out].view(H, total_q, msb)
    assert not bool(torch.isnan(score).any()), "an element of score was not written (or a masked key was read)"
    return score


def run_capi_select(score, lens, topk, bs, fused, expect=0):
    L = lib()
    H, T, nblk = score.shape
    width = topk + int(fused)
    n_out = H * T * max(width, 0)
    flat = torch.full((n_out + 64,), -77, dtype=torch.int32, device="cuda")
    rc = L.mi_prefill_topk_from_score(ptr(score), score.stride(0), score.stride(1), score.stride(2), ptr(lens) if lens is not None else None,
                                      is64(lens), ptr(flat), H, T, nblk, topk, bs, int(fused), stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((flat[n_out:] == -77).all()), "wrote behind the output"
    if expect:
        assert bool((flat == -77).all())
        return None
    return flat[:n_out].view(H, T, width)


def op_score(g, query_pos=None, score_type=None):
    return torch.ops.npu.gqa_prefill_block_score(g["q"], g["k"], g["cu_seqlens"], g["seq_lens"], g["req_to_token"], g["req_pool_indices"],
                                                 g["max_seqlen"], g["sm_scale"], (score_type or g["score_type"]) == "lse", query_pos)


def run_python(g, per_query_seq_lens=None, block_size_q=8, score_type=None, **kw):
    from sgl_kernel_npu.indexer.flash_block_score_prefill import flash_prefill_bnsd_with_topk_idx
    return flash_prefill_bnsd_with_topk_idx(g["q"], g["k"], g["cu_seqlens"], g["seq_lens"], g["req_to_token"], g["req_pool_indices"], block_size_q,
                                            g["block_size"], g["topk"], g["sm_scale"], score_type or g["score_type"],
                                            per_query_seq_lens=per_query_seq_lens, **kw)


# ---- stored outputs of the reference kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ["a", "b", "c"])
def test_against_reference_kernel_outputs(letter):
    """Through the op with query_pos = the packed index (the reference's convention); a -- where that is the true position -- through the
    public function as well, which passes no positions."""
    c = golden(letter)
    g = to_gpu(c)
    packed = torch.arange(c["total_q"], dtype=torch.int64, device="cuda")
    pq = g.get("per_query_seq_lens")
    for qp in ([packed, packed.to(torch.int32), None] if letter == "a" else [packed]):
        score = op_score(g, qp)
        P.check_scores(score.cpu().numpy(), c["score"], tol=P.TOL)
        idx = torch.ops.npu.prefill_topk_from_score(score, pq, c["topk"], c["block_size"], c["fused"])
        P.check_golden_rows(idx.cpu(), c)
    P.check_scores(run_capi_score(g, query_pos=packed).cpu().numpy(), c["score"], tol=P.TOL)
    if letter == "a":
        for bsq in (c["block_size_q"], 1):
            P.check_golden_rows(run_python(g, pq, block_size_q=bsq).cpu(), c)
            P.check_golden_rows(run_python(g, pq, block_size_q=bsq, max_seqlen=c["max_seqlen"]).cpu(), c)


def test_selection_alone_is_bit_equal_to_the_reference():
    from sgl_kernel_npu.indexer.flash_block_score_prefill import flash_prefill_bnsd_topk_from_score
    c = golden("d")
    score, lens = torch.from_numpy(c["score"]).cuda(), c["per_query_seq_lens"].cuda()
    for got in (run_capi_select(score, lens, c["topk"], c["block_size"], True), flash_prefill_bnsd_topk_from_score(score, lens, c["topk"], c["block_size"]),
                run_capi_select(score, lens.to(torch.int64), c["topk"], c["block_size"], True),
                run_capi_select(score.transpose(1, 2).contiguous().transpose(1, 2), lens, c["topk"], c["block_size"], True)):      # a strided score
        assert np.array_equal(got.cpu().numpy(), c["want"])
    plain = run_capi_select(score, None, c["topk"], c["block_size"], False)
    assert np.array_equal(plain.cpu().numpy(), P.select_plain_ref(c["score"], c["topk"]))
    wide = run_capi_select(score, lens, 40, c["block_size"], True)      # topk above the block count
    assert np.array_equal(wide.cpu().numpy(), P.topk_from_score_ref(c["score"], c["per_query_seq_lens"], 40, c["block_size"]))


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES, ids=[c[0] for c in P.CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_against_restatement(case, dtype):
    c = P.make_case(*case, dtype)
    g = to_gpu(c)
    lens = P.causal_lens(c["cu_seqlens"], c["seq_lens"], c["total_q"])
    dlens = torch.from_numpy(lens).cuda()
    for st in ("max", "lse"):
        want = restated((case[0], dtype), c, st)
        score = run_capi_score(g, st)                           # NaN-filled buffer: every element written, no masked key read
        P.check_scores(score.cpu().numpy(), want)
        assert torch.equal(score, op_score(g, None, st))
        plain = run_capi_select(score, None, c["topk"], c["block_size"], False)
        P.check_rows(plain.cpu(), want, c["topk"])
        fused = run_capi_select(score, dlens, c["topk"], c["block_size"], True)
        P.check_rows(fused.cpu(), want, c["topk"], fused_lens=lens, block_size=c["block_size"])
        assert torch.equal(fused[:, :, :c["topk"]], plain), "true positions: no entry is turned into -1"
    own = c["q"].shape[1] == c["k"].shape[2]
    py = run_python(g, dlens if own else None)
    assert torch.equal(py, run_capi_select(op_score(g), dlens if own else None, c["topk"], c["block_size"], own))


@pytest.mark.parametrize("name", ["g4_bs64_lse", "hkv2_g4_d256", "mha_two_runs"])
def test_masked_keys_unowned_pages_and_unused_map_entries_do_not_matter(name):
    case = next(c for c in P.CASES if c[0] == name)
    c = P.make_case(*case, torch.float16)
    assert bool(torch.isnan(c["k_base"]).any()) and bool((c["req_to_token"] == c["poison"] * c["block_size"]).any())
    clean = dict(c, k_base=torch.nan_to_num(c["k_base"], nan=0.0))
    clean["k"] = clean["k_base"][..., :c["k"].shape[-1]]
    clean["req_to_token"] = torch.where(c["req_to_token"] == c["poison"] * c["block_size"], 0, c["req_to_token"])
    a, b = run_capi_score(to_gpu(c)), run_capi_score(to_gpu(clean))
    assert torch.equal(a, b) and bool(torch.isfinite(a).any())
    assert torch.equal(run_capi_select(a, None, c["topk"], c["block_size"], False), run_capi_select(b, None, c["topk"], c["block_size"], False))


def test_tiling_knobs_change_nothing():
    from sgl_kernel_npu.indexer.flash_block_score_prefill import flash_prefill_bnsd_score
    g = to_gpu(P.make_case(*P.CASES[1], torch.bfloat16))
    args = (g["q"], g["k"], g["cu_seqlens"], g["seq_lens"], g["req_to_token"], g["req_pool_indices"])
    base_s = flash_prefill_bnsd_score(*args, 1, g["block_size"], g["sm_scale"], "lse")
    base_i = run_python(g, block_size_q=1)
    for bsq in (8, 64):
        assert torch.equal(base_s, flash_prefill_bnsd_score(*args, bsq, g["block_size"], g["sm_scale"], "lse", num_score_chunks=3, qblock_mappings=(None,) * 6))
        assert torch.equal(base_i, run_python(g, block_size_q=bsq, qblock_mappings=(None,) * 6))


def decode_prefill_pair(B, H, Hkv, D, bs, lens, max_seqblock, topk, dtype, seed):
    """One problem in both forms: a decode batch (req_to_token form), and the same requests as one query token each at position len - 1."""
    gen = torch.Generator().manual_seed(seed)
    used = [-(-n // bs) for n in lens]
    pages = torch.randperm(sum(used), generator=gen).tolist()
    k = torch.randn((sum(used), bs, Hkv, D), generator=gen).to(dtype).cuda()
    q = torch.randn((B, H, D), generator=gen).to(dtype).cuda()
    rtt = torch.zeros((B, max_seqblock * bs), dtype=torch.int32)
    for b in range(B):
        for j in range(used[b]):
            rtt[b, j * bs:(j + 1) * bs] = pages.pop() * bs + torch.arange(bs)
    both = dict(q=q, k=k, seq_lens=torch.tensor(lens, dtype=torch.int32).cuda(), req_to_token=rtt.cuda(), max_seqlen=max_seqblock * bs,
                req_pool_indices=torch.arange(B, dtype=torch.int32).cuda(), block_size=bs, sm_scale=float(D) ** -0.5)
    decode = dict(both, topk=topk, init_blocks=0, local_blocks=0, max_num_blocks=max_seqblock, num_pages=sum(used))
    return decode, dict(both, cu_seqlens=torch.arange(B + 1, dtype=torch.int32).cuda()), used


@pytest.mark.parametrize("shape,score_types", [
    ((2, 8, 2, 64, 16, [597, 203], 40, 4, torch.bfloat16), ("max", "lse")),       # 38 and 13 blocks, the last partial: the masked path
    ((1, 4, 1, 256, 128, [700], 6, 2, torch.float16), ("lse",)),                  # head dim 256: stages of two units
], ids=["g4_d64_bs16", "d256_bs128"])
def test_decode_and_prefill_scores_agree(shape, score_types):
    """The decode and the prefill indexer run one score engine: a block's score is the same bits in both.  Every MFMA output column is its
    own dot product, the per-lane sum order is the same and the run partition does not enter a block's score.  Blocks behind a request's
    end are -inf in the prefill form and unwritten in the decode form: not compared."""
    from test_block_score_gpu import run_capi as run_decode_capi
    decode, prefill, used = decode_prefill_pair(*shape, seed=11)
    for st in score_types:
        _, dec = run_decode_capi(dict(decode, score_type=st))   # [B, H, max_seqblock]
        pre = run_capi_score(prefill, st)                       # [H, B, max_seqblock]
        for b, nb in enumerate(used):
            assert torch.equal(dec[b, :, :nb], pre[:, b, :nb]), (st, b, (dec[b, :, :nb] != pre[:, b, :nb]).nonzero().tolist())


# ---- with the attention kernels ------------------------------------------------------------------------------------------------------------
def dense_causal_ref(c, round_p=None):
    """float64 softmax attention of every token over the keys 0 .. position of its request; round_p: P rounded to that dtype before P.V."""
    q, k, v = c["q"].double(), c["k"].double(), c["v"].double()
    bs, rtt, pool = c["block_size"], c["req_to_token"].long(), c["req_pool_indices"].long()
    pos = P.true_positions(c["cu_seqlens"], c["seq_lens"], c["total_q"])
    out = torch.zeros(q.shape, dtype=torch.float64)
    for r in range(len(c["seq_lens"])):
        for t in range(int(c["cu_seqlens"][r]), int(c["cu_seqlens"][r + 1])):
            n = int(pos[t]) + 1
            slots = rtt[pool[r], :n]
            kk, vv = k[slots // bs, slots % bs, 0], v[slots // bs, slots % bs, 0]
            s = (q[t] @ kk.T) * c["sm_scale"]
            p = torch.exp(s - s.max(dim=1, keepdim=True).values)
            pr = p.to(round_p).double() if round_p is not None else p
            out[t] = (pr @ vv) / p.sum(dim=1, keepdim=True)
    return out


def attention_refs(c, dtype):
    exact = dense_causal_ref(c)
    return exact, (exact if dtype == torch.float16 else dense_causal_ref(c, round_p=dtype)).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_end_to_end_with_the_block_sparse_prefill_attention(dtype):
    """Fused form with topk >= every row's visible blocks, one index head on the one kv head: every visible block once plus the appended
    slot, so the block-sparse prefill attention over the list is dense causal attention."""
    from sgl_kernel_npu.attention.fia_blockq_attention import flash_prefill_bnsd_blockq_sparse_fia
    from test_block_score_gpu import check_attention
    c = P.attention_case(dtype)
    g = to_gpu(c)
    bs, topk = c["block_size"], c["topk"]
    lens = P.causal_lens(c["cu_seqlens"], c["seq_lens"], c["total_q"])
    assert -(-int(lens.max()) // bs) <= topk and topk + 1 <= 64
    dlens = torch.from_numpy(lens).cuda()
    gi = dict(g, q=g["q"][:, :1])                               # the index head: a strided view of the first attention head
    idx = run_python(gi, dlens, max_seqlen=c["max_seqlen"])
    assert idx.shape == (1, c["total_q"], topk + 1)
    want = restated(("attention", dtype), dict(c, q=c["q"][:, :1]))
    P.check_rows(idx.cpu(), want, topk, fused_lens=lens, block_size=bs)
    owner = torch.repeat_interleave(g["req_pool_indices"], (g["cu_seqlens"][1:] - g["cu_seqlens"][:-1]).long())
    got = flash_prefill_bnsd_blockq_sparse_fia(g["q"], g["k"], g["v"], idx, dlens, owner, g["req_to_token"], bs, c["sm_scale"], c["k"].shape[0],
                                               -(-c["max_seqlen"] // bs))
    torch.cuda.synchronize()
    exact, ref = attention_refs(c, dtype)
    check_attention(got, ref, exact, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_indexer_form_returns_dense_causal_attention_by_composition(dtype):
    from sgl_kernel_npu.indexer.flash_block_score_prefill import flash_prefill_bnsd_indexer
    from test_block_score_gpu import check_attention
    c = P.attention_case(dtype)
    g = to_gpu(c)
    idx_o, idx = flash_prefill_bnsd_indexer(g["q"], g["k"], g["v"], g["cu_seqlens"], g["seq_lens"], g["req_to_token"], g["req_pool_indices"], 8,
                                            c["block_size"], 3, c["sm_scale"], "max", max_seqlen=c["max_seqlen"])
    torch.cuda.synchronize()
    P.check_rows(idx.cpu(), restated(("attention4", dtype), c), 3)
    exact, ref = attention_refs(c, dtype)
    check_attention(idx_o, ref, exact, dtype)


def test_captured_in_a_graph_follows_new_requests():
    """Nothing is read back on the host when max_seqlen is given: captured once, replayed after cu_seqlens, seq_lens, the map, the pool
    rows and q changed in place."""
    problems = P.graph_cases()
    g = to_gpu(problems[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_python(g, max_seqlen=512)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run_python(g, max_seqlen=512)
    for i, p in enumerate(problems):
        for key in ("cu_seqlens", "seq_lens", "req_to_token", "req_pool_indices", "q"):
            g[key].copy_(p[key])
        out.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        assert torch.equal(replayed, run_python(g, max_seqlen=512)), i
        P.check_rows(replayed.cpu(), restated(("graph", i), p), p["topk"])


def test_at_the_declared_limits():
    c = P.limits_case()
    g = to_gpu(c)
    want = restated("limits", c)
    score = run_capi_score(g)
    assert score.shape == (1, 2, 16384)
    P.check_scores(score.cpu().numpy(), want)
    lens = P.causal_lens(c["cu_seqlens"], c["seq_lens"], 2)
    P.check_rows(run_python(g, max_seqlen=c["max_seqlen"]).cpu(), want, 1024)
    P.check_rows(run_python(g, torch.from_numpy(lens).cuda(), max_seqlen=c["max_seqlen"]).cpu(), want, 1024, fused_lens=lens, block_size=16)


def test_argument_checks_and_limits():
    g = to_gpu(P.make_case(*P.CASES[1], torch.float16))
    run_capi_score(g)                                           # the case itself is served
    for over in (dict(max_seqblock=16385), dict(max_seqblock=0), dict(block_size=48), dict(head_dim=60), dict(head_dim=264), dict(sm_scale=0.0),
                 dict(kv_heads=3), dict(heads=0)):
        run_capi_score(g, expect=EINVAL, **over)
    score, lens = torch.zeros((2, 5, 7), device="cuda"), torch.ones(5, dtype=torch.int32, device="cuda")
    run_capi_select(score, lens, 1025, 16, True, expect=EINVAL)
    run_capi_select(score, lens, 0, 16, True, expect=EINVAL)
    run_capi_select(score, None, 2, 16, True, expect=EINVAL)    # the fused form needs the lengths
    run_capi_select(score, lens, 2, 0, True, expect=EINVAL)
    with pytest.raises(RuntimeError):
        op_score(dict(g, max_seqlen=64 * 16384 + 1))
    with pytest.raises(RuntimeError):
        op_score(dict(g, k=g["k"][..., :64]))                   # head dims differ
    with pytest.raises(RuntimeError):
        op_score(dict(g, seq_lens=g["seq_lens"][:-1]))
    with pytest.raises(RuntimeError):
        torch.ops.npu.prefill_topk_from_score(score, None, 2, 16, True)
    with pytest.raises(RuntimeError):
        torch.ops.npu.prefill_topk_from_score(score, lens, 1025, 16, True)
    empty = run_python(dict(g, topk=0))
    assert empty.shape == (4, g["q"].shape[0], 0) and empty.is_cuda
