"""GPU parity of block-sparse attention over per-token block lists (C-ABI mi_sparse_attention_score and
torch.ops.npu.npu_sparse_attention_score) against the float64 restatement (tests/sparse_attention_score_ref.py), at the criterion of
test_gqa_sparse_decode_gpu.check.

Every C-ABI run keeps sentinels behind the output and the workspace.  Every table entry that must not be used -- blocks behind a request's
kv length -- names a page of NaNs that lies inside the cache allocation, and every scale that must not be used is NaN: a read through such an
entry shows as a wrong value, never as a fault.  Block tables are exactly [batch, columns], so an id that must not be looked up (10**6 behind
the live prefix) would leave the table."""
import ctypes
from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p

import pytest
import torch

from capi import load, stream_ptr
from sparse_attention_score_ref import sparse_attention_score_ref

pytestmark = pytest.mark.gpu
EINVAL = -1
FP8 = torch.float8_e4m3fn
DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1, FP8: 3}
JUNK = 10 ** 6


class Params(ctypes.Structure):
    """mi_sparse_attention_score_params of include/mi_sgl_kernels.h"""
    _fields_ = ([(n, c_void_p) for n in ("q", "k", "v", "out", "select_idx", "select_num_idx", "block_table", "actual_seq_lengths",
                                         "actual_seq_lengths_kv", "q_dequant_scale", "k_dequant_scale", "v_dequant_scale", "workspace")]
                + [("workspace_bytes", c_size_t), ("tokens", c_int64)]
                + [(n, c_int64) for n in ("q_stride_t", "q_stride_h", "k_stride_blk", "k_stride_row", "k_stride_h", "v_stride_blk", "v_stride_row",
                                          "v_stride_h", "o_stride_t", "o_stride_h", "idx_stride_h", "idx_stride_q", "idx_stride_k", "num_stride_h",
                                          "num_stride_q", "bt_stride_b", "bt_stride_n")]
                + [(n, c_int) for n in ("batch", "q_heads", "kv_heads", "head_dim", "block_size", "topk", "columns", "num_pages", "q_scale_blocks",
                                        "dtype", "num_chunks")]
                + [("sm_scale", c_float)])


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load("libmi_sgl_kernels.so")
        _lib.mi_sparse_attention_score_workspace.restype = c_size_t
        _lib.mi_sparse_attention_score_workspace.argtypes = [c_int64, c_int, c_int, c_int]
        _lib.mi_sparse_attention_score_num_chunks.argtypes = [c_int64, c_int, c_int]
        _lib.mi_sparse_attention_score.argtypes = [ctypes.POINTER(Params), c_void_p]
    return _lib


def out_dtype(c):
    return torch.float16 if c["q"].dtype == FP8 else c["q"].dtype


def run_capi(c, num_chunks, expect=0, **override):
    """c: a make_case dict.  Returns the output; asserts the sentinels behind output and workspace."""
    L = lib()
    q, k, v, idx, bt, num = c["q"], c["k"], c["v"], c["select_idx"], c["block_table"], c.get("select_num_idx")
    T, Hq, D = q.shape
    Hkv, topk = idx.shape[0], idx.shape[2]
    nc = num_chunks
    if not nc:                                                 # the library's choice: a power of two within the list
        nc = L.mi_sparse_attention_score_num_chunks(T, Hkv, topk)
        assert nc >= 1 and nc & (nc - 1) == 0 and nc <= topk, nc
    wsb = L.mi_sparse_attention_score_workspace(T, Hq, D, nc)
    assert (wsb == 0) == (nc == 1)
    tail = 256
    ws = torch.full((wsb + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    flat = torch.full((T * Hq * D + tail,), -77.0, dtype=out_dtype(c), device="cuda")
    out = flat[:T * Hq * D].view(T, Hq, D)
    p = Params()
    p.q, p.k, p.v, p.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.select_idx, p.block_table = idx.data_ptr(), bt.data_ptr()
    p.select_num_idx = num.data_ptr() if num is not None else None
    p.actual_seq_lengths = c["q_lens"].data_ptr() if c.get("q_lens") is not None else None
    p.actual_seq_lengths_kv = c["kv_lens"].data_ptr()
    if "sq" in c:
        p.q_dequant_scale, p.k_dequant_scale, p.v_dequant_scale = c["sq"].data_ptr(), c["sk"].data_ptr(), c["sv"].data_ptr()
        p.q_scale_blocks = c["sq"].shape[2]
    p.workspace, p.workspace_bytes, p.tokens = ws.data_ptr(), wsb, T
    p.q_stride_t, p.q_stride_h = q.stride(0), q.stride(1)
    p.k_stride_blk, p.k_stride_row, p.k_stride_h = k.stride(0), k.stride(1), k.stride(2)
    p.v_stride_blk, p.v_stride_row, p.v_stride_h = v.stride(0), v.stride(1), v.stride(2)
    p.o_stride_t, p.o_stride_h = out.stride(0), out.stride(1)
    p.idx_stride_h, p.idx_stride_q, p.idx_stride_k = idx.stride()
    if num is not None:
        p.num_stride_h, p.num_stride_q = num.stride()
    p.bt_stride_b, p.bt_stride_n = bt.stride()
    p.batch, p.q_heads, p.kv_heads, p.head_dim, p.block_size, p.topk = bt.shape[0], Hq, Hkv, D, k.shape[1], topk
    p.columns, p.num_pages, p.dtype, p.num_chunks, p.sm_scale = bt.shape[1], k.shape[0], DTYPE_CODE[q.dtype], num_chunks, c["scale"]
    for key, val in override.items():
        setattr(p, key, val)
    rc = L.mi_sparse_attention_score(ctypes.byref(p), stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((flat[T * Hq * D:] == -77.0).all()), "wrote behind the output"
    assert bool((ws[wsb:] == 0xA5).all()), "wrote behind the workspace"
    return out


def op_args(c):
    kw = dict(select_num_idx=c.get("select_num_idx"), actual_seq_lengths=c.get("q_lens"), actual_seq_lengths_kv=c["kv_lens"],
              num_key_value_heads=c["select_idx"].shape[0], scale_value=c["scale"], block_size=c["k"].shape[1], top_k=c["select_idx"].shape[2],
              inner_precise=4)
    if "sq" in c:
        kw.update(q_dequant_scale=c["sq"], k_dequant_scale=c["sk"], v_dequant_scale=c["sv"])
    return (c["q"], c["k"], c["v"], c["select_idx"], c["block_table"]), kw


def the_op():
    import sgl_kernel_npu  # noqa: F401  (loads the operator library)
    return torch.ops.npu.npu_sparse_attention_score


def run_op(c):
    args, kw = op_args(c)
    out = the_op()(*args, **kw)
    torch.cuda.synchronize()
    return out


def restate(c, rounded=False):
    """exact, or what the kernel rounds: P to the engine dtype (fp16 for FP8 inputs) and, with FP8, the dequantised value rows to fp16."""
    engine = out_dtype(c)
    kw = dict(select_num_idx=c.get("select_num_idx"), actual_seq_lengths=c.get("q_lens"), actual_seq_lengths_kv=c["kv_lens"], scale_value=c["scale"],
              q_dequant_scale=c.get("sq"), k_dequant_scale=c.get("sk"), v_dequant_scale=c.get("sv"))
    if rounded:
        kw.update(round_p=engine, fold_sv=torch.float16 if "sq" in c else None)
    return torch.from_numpy(sparse_attention_score_ref(c["q"], c["k"], c["v"], c["select_idx"], c["block_table"], **kw))


def check(got, want, exact, dtype):
    """test_gqa_sparse_decode_gpu.check.  fp16: against `want` at atol = 1e-3, rtol = 2**-10.  bf16 and FP8: kernel and `want` round alike
    but against different running maxima, so both are measured against the exact float64 result."""
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


class Refs:
    """The two restatements of a case, computed once."""

    def __init__(self, c):
        self.dtype = c["q"].dtype
        self.exact = restate(c)
        want = restate(c, rounded=True)
        self.want = want if self.dtype == torch.float16 else want.to(out_dtype(c))

    def check(self, got):
        check(got, self.want, self.exact, self.dtype)


def chunk_counts(topk):
    """0 = the helper's own choice on this machine, and every power of two it can return on any machine (up to topK and 64)."""
    return [0] + [n for n in (1, 2, 4, 8, 16, 32, 64) if n <= topk]


def check_all_entries(c, chunks=None):
    r = Refs(c)
    topk = c["select_idx"].shape[2]
    for n in chunk_counts(topk) if chunks is None else chunks:
        if n <= topk:
            print("chunks", n)
            r.check(run_capi(c, n))
    print("torch.ops.npu")
    r.check(run_op(c))
    return r


def make_case(q_lens, kv_lens, Hq, Hkv, D, bs, topk, dtype, seed, T=None, Q=None, columns=None, counts=None, pass_q_lens=True):
    """A problem on the GPU.  Lists: a random subset of the logical blocks 0 .. columns + 1 (so: some behind the token's diagonal block, some
    behind the table) in random slots, -1 elsewhere; the diagonal block is in the list with probability 3/4, anywhere; one duplicate where
    there is room.  counts: None = no select_num_idx; "full" = topK everywhere; "prefix" = a random count per (kv head, token) -- 0 for token
    1, above topK for token 2, negative for token 3 -- with JUNK in every slot behind it.  T rows of query (default: the sum of q_lens; more = padding tokens), Q rows of
    lists (default T)."""
    g = torch.Generator().manual_seed(seed)
    batch = len(kv_lens)
    total = sum(q_lens)
    T = total if T is None else T
    Q = T if Q is None else Q
    if columns is None:
        columns = max(1, (max(kv_lens) + bs - 1) // bs)
    fp8 = dtype == FP8
    num_pages = batch * columns + 1
    poison = num_pages - 1                                     # inside the allocation, named by every table entry that must not be used
    pages = torch.randperm(num_pages - 1, generator=g).reshape(batch, columns)
    bt = torch.full((batch, columns), poison, dtype=torch.int32)
    for b in range(batch):
        for lb in range(columns):
            if lb * bs < kv_lens[b]:
                bt[b, lb] = pages[b, lb]
    kf, vf = torch.randn((num_pages, bs, Hkv, D), generator=g), torch.randn((num_pages, bs, Hkv, D), generator=g)
    qf = torch.randn((T, Hq, D), generator=g)
    where = []                                                 # (request, position) of every real token
    for b in range(batch):
        where += [(b, kv_lens[b] - q_lens[b] + j) for j in range(q_lens[b])]
    c = dict(scale=float(D) ** -0.5)
    if fp8:                                                    # per (request, kv head, block) and per (request, q head, q block): scale = absmax / 448
        nqb = columns
        sk, sv = torch.full((batch, Hkv, columns), float("nan")), torch.full((batch, Hkv, columns), float("nan"))
        sq = torch.full((batch, Hq, nqb), float("nan"))
        k, v, q = torch.zeros_like(kf).to(FP8), torch.zeros_like(vf).to(FP8), torch.zeros_like(qf).to(FP8)
        for b in range(batch):
            for lb in range(columns):
                pg = int(bt[b, lb])
                if pg == poison:
                    continue
                sk[b, :, lb] = kf[pg].abs().amax(dim=(0, 2)) / 448
                sv[b, :, lb] = vf[pg].abs().amax(dim=(0, 2)) / 448
                k[pg] = (kf[pg] / sk[b, :, lb, None]).to(FP8)
                v[pg] = (vf[pg] / sv[b, :, lb, None]).to(FP8)
        for t, (b, pos) in enumerate(where):
            if pos >= 0:
                rows = [u for u, (b2, p2) in enumerate(where) if b2 == b and p2 >= 0 and p2 // bs == pos // bs]
                sq[b, :, pos // bs] = qf[rows].abs().amax(dim=(0, 2)) / 448
                q[t] = (qf[t] / sq[b, :, pos // bs, None]).to(FP8)
        nan8 = torch.full((bs, Hkv, D), float("nan")).to(FP8)
        k[poison], v[poison] = nan8, nan8
        c.update(sq=sq.cuda(), sk=sk.cuda(), sv=sv.cuda())
    else:
        k, v, q = kf.to(dtype), vf.to(dtype), qf.to(dtype)
        k[poison], v[poison] = float("nan"), float("nan")
    idx = torch.full((Hkv, Q, topk), -1, dtype=torch.int32)
    num = torch.full((Hkv, Q), topk, dtype=torch.int32)
    for kh in range(Hkv):
        for t in range(Q):
            cand = torch.randperm(columns + 2, generator=g)[:max(1, (2 * topk) // 3)].tolist()
            if t < total and where[t][1] >= 0:
                diag = where[t][1] // bs
                if int(torch.randint(0, 4, (1,), generator=g)) and diag not in cand:
                    cand[0] = diag
            slots = torch.randperm(topk, generator=g)[:len(cand)].tolist()
            for s, blk in zip(slots, cand):
                idx[kh, t, s] = blk
            if topk >= 2:
                idx[kh, t, (slots[0] + 1) % topk] = idx[kh, t, slots[0]]
            if counts == "prefix":
                n = {1: 0, 2: topk + 2, 3: -1}.get(t, int(torch.randint(1, topk + 1, (1,), generator=g)))
                num[kh, t] = n
                idx[kh, t, min(max(n, 0), topk):] = JUNK
    c.update(q=q.cuda(), k=k.cuda(), v=v.cuda(), select_idx=idx.cuda(), block_table=bt.cuda(), kv_lens=torch.tensor(kv_lens, dtype=torch.int32).cuda())
    if pass_q_lens:
        c["q_lens"] = torch.tensor(q_lens, dtype=torch.int32).cuda()
    if counts is not None:
        c["select_num_idx"] = num.cuda()
    return c


M3 = dict(Hq=8, Hkv=1, D=128, bs=128, topk=17)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("pass_q_lens", [True, False])
def test_m3_decode(dtype, pass_q_lens):
    """One token per request, kv lengths of one key, one key in the second block and several blocks; with and without actual_seq_lengths."""
    check_all_entries(make_case([1, 1, 1], [1, 129, 700], dtype=dtype, seed=1, pass_q_lens=pass_q_lens, **M3))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_verify_across_a_block_boundary(dtype):
    """The request of kv 130, q 4 has its tokens at positions 126 .. 129: the diagonal block changes from 0 to 1 between them.  Around it
    requests of 1 and 3 tokens and, in the middle, one of none."""
    c = make_case([1, 4, 0, 3], [300, 130, 50, 260], dtype=dtype, seed=2, counts="full", **M3)
    r = check_all_entries(c)
    # token 1 + 1 (position 127) sees nothing of block 1, token 1 + 2 (position 128) its first key: rows differ from their neighbours'
    assert not torch.equal(r.exact[2], r.exact[3])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Hq,Hkv,D,bs,topk,q_lens,kv_lens", [
    (16, 2, 128, 64, 9, [2, 1, 3], [200, 64, 385]),
    (64, 8, 128, 64, 6, [1, 2], [129, 300]),
    (8, 2, 64, 16, 12, [3, 1, 2], [100, 17, 160]),             # four blocks share a 64-key tile
    (8, 2, 80, 32, 5, [2, 2], [70, 33]),                       # padded head dim
])
def test_other_group_sizes(Hq, Hkv, D, bs, topk, q_lens, kv_lens, dtype):
    check_all_entries(make_case(q_lens, kv_lens, Hq, Hkv, D, bs, topk, dtype, seed=Hq + topk, counts="full"))


@pytest.mark.parametrize("batch", [70, 300])
def test_many_requests(batch):
    """More requests than a wave has lanes: a lane owns 2 (batch 70) or 5 (batch 300: more than it keeps in registers) of them.  Query
    lengths 0 .. 3, every token of every request at its own position."""
    q_lens = [(7 * i) % 4 for i in range(batch)]
    kv_lens = [q + (13 * i) % 40 for i, q in enumerate(q_lens)]
    c = make_case(q_lens, kv_lens, 8, 2, 64, 16, 4, torch.float16, seed=batch, T=sum(q_lens) + 3, counts="prefix")
    check_all_entries(c, chunks=(0, 2))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_slots_behind_the_live_prefix_are_never_looked_at(dtype):
    """select_num_idx below topK with ids of 10**6 behind the prefix: looking one up would leave the [batch, columns] table.  The result is
    the clean list's, bit for bit at the same chunk count."""
    c = make_case([2, 1, 3], [500, 129, 700], dtype=dtype, seed=4, counts="prefix", **M3)
    idx, num = c["select_idx"], c["select_num_idx"]
    assert bool((idx == JUNK).any()) and bool((num <= 0).any()) and bool((num > 17).any()) and c["block_table"].is_contiguous()
    clean = dict(c, select_idx=torch.where(idx == JUNK, torch.full_like(idx, -1), idx))
    r = check_all_entries(c)
    for n in (1, 2, 4):
        assert torch.equal(run_capi(c, n), run_capi(clean, n)), n
    assert torch.equal(run_op(c), run_op(clean))
    for kh, t in (num <= 0).nonzero().tolist():                # a count of 0 (or below): a zeros row
        assert bool((r.exact[t] == 0).all()) and bool((run_op(c)[t] == 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_a_count_below_topk_cuts_off_blocks_that_would_contribute(dtype):
    """Every slot, before and behind the count, holds a block at or before the token's diagonal block: whole ones and the diagonal one, which
    stands right behind the prefix (even tokens) or inside it and again right behind it (odd tokens).  Only the count keeps the slots behind it
    out.  Counts 1, 5, 9, 12, 16, 8 of 17 slots with 1, 2, 4, 8 and 16 chunks (17, 9, 5, 3, 2 slots each): the prefix ends inside the first
    chunk, inside a later one, and on a chunk's edge; chunks wholly behind it are empty."""
    q_lens, kv_lens, counts = [2, 1, 3], [900, 700, 1300], [1, 5, 9, 12, 16, 8]
    c = make_case(q_lens, kv_lens, dtype=dtype, seed=14, counts="full", **M3)
    g = torch.Generator().manual_seed(15)
    pos = [kv - ql + j for ql, kv in zip(q_lens, kv_lens) for j in range(ql)]
    idx, num = c["select_idx"].cpu(), c["select_num_idx"].cpu()
    for t, (at, n) in enumerate(zip(pos, counts)):
        diag = at // 128
        idx[0, t] = torch.randint(0, diag, (17,), generator=g).to(torch.int32)      # whole blocks before the diagonal one
        idx[0, t, n] = diag
        if t % 2:
            idx[0, t, 0] = diag
        num[0, t] = n
    c["select_idx"], c["select_num_idx"] = idx.cuda(), num.cuda()
    cut = idx.clone()
    for t, n in enumerate(counts):
        cut[0, t, n:] = -1
    truncated = dict(c, select_idx=cut.cuda())
    whole = dict(c, select_num_idx=None)
    r = check_all_entries(c)
    assert torch.equal(r.exact, restate(truncated)) and not torch.allclose(r.exact, restate(whole), atol=1e-2)
    for n in chunk_counts(17):
        got = run_capi(c, n)
        assert torch.equal(got, run_capi(truncated, n)), n
        assert not torch.allclose(got.float(), run_capi(whole, n).float(), atol=1e-2), n
    assert torch.equal(run_op(c), run_op(truncated))


def test_list_contents():
    """-1 inside the prefix, duplicates, a count of 0, only blocks behind the causal end, only blocks behind the table."""
    c = make_case([2, 2], [300, 200], 8, 2, 64, 32, 6, torch.float16, seed=5, counts="full")
    idx, num = c["select_idx"], c["select_num_idx"]
    row = lambda *ids: torch.tensor(ids, dtype=torch.int32, device="cuda")
    idx[0, 0] = row(-1, 3, -1, 3, 0, -1)                       # token 0: request 0 at position 298: block 3 twice and block 0
    idx[1, 0] = row(2, 2, 2, 2, 2, 2)
    num[0, 1] = 0
    idx[1, 1] = row(-1, -1, -1, -1, -1, -1)
    idx[0, 2] = row(7, 8, 9, 7, 8, 9)                          # token 2: request 1 at position 198: diagonal block 6, all of these lie behind it
    idx[1, 2] = row(6, 7, -1, 0, 9, 6)                         # the diagonal block twice, block 0, two behind
    idx[0, 3] = row(10, 11, 12, 13, 10 ** 6, 2 ** 31 - 1)      # behind the table's 10 columns
    r = check_all_entries(c)
    for n in (0, 1, 2, 4):
        got = run_capi(c, n).cpu()
        assert bool((got[1, 0:4] == 0).all()) and bool((got[1, 4:8] == 0).all()) and bool((got[2, 0:4] == 0).all()) and bool((got[3, 0:4] == 0).all())
        assert bool((got[0] != 0).any()) and bool((got[2, 4:8] != 0).any())
    assert bool((r.exact[2, 0:4] == 0).all()) and bool((r.exact[3, 0:4] == 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_padding_rows_and_tokens(dtype):
    """Q > T (the lists are a graph buffer's), T above the sum of the lengths (zeros rows), a request whose first tokens stand before
    position 0 (zeros rows)."""
    c = make_case([2, 3, 1], [400, 2, 129], dtype=dtype, seed=6, T=9, Q=12, counts="prefix", **M3)
    r = check_all_entries(c)
    got = run_op(c)
    assert bool((got[6:] == 0).all()) and bool((got[2] == 0).all())      # behind the sum; request 1's token 0 at position 2 - 3 + 0 = -1
    assert bool((r.exact[6:] == 0).all()) and bool((r.exact[2] == 0).all()) and bool((r.exact[0] != 0).any())


@pytest.mark.parametrize("form", ["decode", "verify"])
def test_fp8(form):
    """float8_e4m3fn q / k / v, fp16 out.  K / V from N(0, 1) quantised per (request, kv head, block) with scale = absmax / 448, q per
    (request, head, q block): every scale distinct, every scale that must not be read NaN."""
    if form == "decode":
        c = make_case([1, 1, 1], [1, 129, 700], dtype=FP8, seed=7, **M3)
    else:
        c = make_case([1, 4, 0, 3], [300, 130, 50, 260], dtype=FP8, seed=8, counts="prefix", **M3)
    assert c["sk"][~c["sk"].isnan()].unique().numel() == int((~c["sk"].isnan()).sum())
    r = check_all_entries(c)
    assert run_op(c).dtype == torch.float16 and r.exact.abs().max() > 0.1
    # the scales matter: with all of them 1 the result is another one
    ones = dict(c, sq=torch.ones_like(c["sq"]), sk=torch.ones_like(c["sk"]), sv=torch.ones_like(c["sv"]))
    assert not torch.allclose(run_op(ones).float(), run_op(c).float(), atol=1e-2, rtol=1e-2)
    # a token whose q block lies behind q_dequant_scale's columns: a zeros row, nothing read
    short = dict(c, sq=c["sq"][:, :, :1].contiguous())
    got = run_op(short).cpu()
    pos = [kv - ql + j for ql, kv in zip(c["q_lens"].tolist(), c["kv_lens"].tolist()) for j in range(ql)]
    for t, at in enumerate(pos):
        if at >= 128:
            assert bool((got[t] == 0).all())
        else:
            assert torch.equal(got[t], run_op(c).cpu()[t])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Hq,Hkv,D,bs,topk,kv_lens", [(8, 1, 128, 128, 17, [1, 129, 700, 1280]), (16, 2, 64, 16, 12, [100, 17, 160])])
def test_decode_form_equals_gqa_share_sparse_decode(Hq, Hkv, D, bs, topk, kv_lens, dtype):
    """One token per request and no count: flash_decode_bnsd_with_gqa_share_sparse (the existing kernel) on the same caches and lists."""
    from sgl_kernel_npu.attention.gqa_share_sparse_attention import flash_decode_bnsd_with_gqa_share_sparse
    c = make_case([1] * len(kv_lens), kv_lens, Hq, Hkv, D, bs, topk, dtype, seed=9, pass_q_lens=False)
    old = flash_decode_bnsd_with_gqa_share_sparse(c["q"], None, c["k"], c["v"], c["block_table"], c["kv_lens"], bs, c["select_idx"], c["scale"])
    torch.cuda.synchronize()
    exact = restate(c)
    check(run_op(c), old.cpu(), exact, dtype)
    for n in (1, 2, 4):
        check(run_capi(c, n), old.cpu(), exact, dtype)


def test_captured_in_a_graph_follows_new_lists_counts_and_lengths():
    """Nothing is read back on the host: the op is captured once and replayed after lists, counts and both lengths changed in place."""
    dtype = torch.float16
    shape = dict(dtype=dtype, T=8, Q=8, columns=6, counts="prefix", **M3)
    c = make_case([1, 4, 2], [300, 130, 700], seed=10, **shape)
    others = [make_case([3, 0, 5], [768, 50, 133], seed=11, **shape), make_case([2, 2, 2], [2, 640, 129], seed=12, **shape)]
    args, kw = op_args(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        the_op()(*args, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = the_op()(*args, **kw)
    for o in [c] + others:                                     # the captured contents, then two other problems of the same shape
        for key in ("q", "k", "v", "select_idx", "select_num_idx", "block_table", "q_lens", "kv_lens"):
            c[key].copy_(o[key])
        out.fill_(9.0)
        graph.replay()
        torch.cuda.synchronize()
        Refs(c).check(out)


def test_argument_checks_raise():
    op = the_op()
    c = make_case([2, 1], [200, 129], 8, 2, 64, 64, 5, torch.float16, seed=13, counts="full")
    f = make_case([2, 1], [200, 129], dtype=FP8, seed=13, counts="full", **M3)
    (q, k, v, idx, bt), kw = op_args(c)
    (fq, fk, fv, fidx, fbt), fkw = op_args(f)
    base = op(q, k, v, idx, bt, **kw)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    bad = [
        lambda: op(q.float(), k, v, idx, bt, **kw),                                            # dtypes
        lambda: op(q, k.to(torch.bfloat16), v, idx, bt, **kw),
        lambda: op(q, k, v.to(torch.bfloat16), idx, bt, **kw),
        lambda: op(q, k, v, idx.long(), bt, **kw),
        lambda: op(q, k, v, idx, bt.long(), **kw),
        lambda: op(q, k, v, idx, bt, **dict(kw, select_num_idx=kw["select_num_idx"].long())),
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths=kw["actual_seq_lengths"].long())),
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths_kv=kw["actual_seq_lengths_kv"].long())),
        lambda: op(q, k, v, idx.cpu(), bt, **kw),                                              # devices
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths_kv=kw["actual_seq_lengths_kv"].cpu())),
        lambda: op(q[0], k, v, idx, bt, **kw),                                                 # ranks
        lambda: op(q, k[0], v[0], idx, bt, **kw),
        lambda: op(q, k, v, idx[0], bt, **kw),
        lambda: op(q, k, v, idx, bt[0], **kw),
        lambda: op(q[:, :7], k, v, idx, bt, **kw),                                             # Hq % Hkv
        lambda: op(q, k, v[:5], idx, bt, **kw),                                                # key.shape == value.shape
        lambda: op(q, k[:, :, :1], v[:, :, :1], idx, bt, **kw),                                # key.size(2) == Hkv
        lambda: op(q, k[..., :32], v[..., :32], idx, bt, **kw),                                # key.size(3) == D
        lambda: op(q, k, v, idx, bt, **dict(kw, block_size=128)),                              # block_size == key.size(1)
        lambda: op(q, k[:, :48], v[:, :48], idx, bt, **dict(kw, block_size=48)),               # ... and one of 16 / 32 / 64 / 128
        lambda: op(q[..., :60], k[..., :60], v[..., :60], idx, bt, **kw),                      # D a multiple of 8
        lambda: op(torch.cat([q] * 5, 2), torch.cat([k] * 5, 3), torch.cat([v] * 5, 3), idx, bt, **kw),      # D <= 256
        lambda: op(q, k, v, idx[:, :2], bt, **dict(kw, select_num_idx=kw["select_num_idx"][:, :2])),         # Q >= T
        lambda: op(q, k, v, idx, bt, **dict(kw, select_num_idx=i32(2, 4))),                    # select_num_idx [Hkv, Q]
        lambda: op(q, k, v, idx, bt, **dict(kw, select_num_idx=i32(3))),
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths=i32(3))),                   # batch elements
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths_kv=i32(1))),
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths_kv=None)),                  # required
        lambda: op(q, k, v, idx, bt, **dict(kw, actual_seq_lengths=None)),                     # T == batch then
        lambda: op(q, k, v, idx[:, :, :0], bt, **kw),                                          # topK >= 1
        lambda: op(q, k, v, i32(2, 3, 1025), bt, **dict(kw, select_num_idx=None)),             # topK <= 1024
        lambda: op(q, k, v, idx, bt, **dict(kw, scale_value=-1.0)),
        lambda: op(q, k, v, idx, bt, **dict(kw, q_dequant_scale=f["sq"], k_dequant_scale=f["sk"], v_dequant_scale=f["sv"])),   # scales without FP8
        lambda: op(fq, fk, fv, fidx, fbt, **dict(fkw, q_dequant_scale=None)),                  # FP8 without its scales
        lambda: op(fq, fk, fv, fidx, fbt, **dict(fkw, k_dequant_scale=None)),
        lambda: op(fq, fk, fv, fidx, fbt, **dict(fkw, v_dequant_scale=None)),
        lambda: op(fq, fk, fv, fidx, fbt, **dict(fkw, k_dequant_scale=f["sk"][:, :, :1])),     # [batch, Hkv, columns]
        lambda: op(fq, fk, fv, fidx, fbt, **dict(fkw, q_dequant_scale=f["sq"].double())),
        lambda: op(fq[..., :64], fk[..., :64], fv[..., :64], fidx, fbt, **fkw),                # FP8: D == 128
        lambda: op(fq, fk[:, :64], fv[:, :64], fidx, fbt, **dict(fkw, block_size=64)),         # FP8: block_size == 128
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} did not raise")
    # T == 0 and batch == 0: empty results
    assert op(q[:0], k, v, idx, bt, **kw).shape == (0, 8, 64)
    empty = op(q[:0], k, v, idx, bt[:0], **dict(kw, actual_seq_lengths=i32(0), actual_seq_lengths_kv=i32(0)))
    assert empty.shape == (0, 8, 64)
    # shapes override the attributes; scale_value 0 is 1 / sqrt(D); every inner_precise is the same path
    assert torch.equal(op(q, k, v, idx, bt, **dict(kw, num_key_value_heads=1, top_k=99, scale_value=0.0, inner_precise=0)), base)
    # the C-ABI refuses what it does not serve, before any launch
    L = lib()
    assert L.mi_sparse_attention_score_workspace(3, 8, 64, 1) == 0 and L.mi_sparse_attention_score_workspace(3, 8, 80, 4) == 3 * 8 * 4 * 130 * 4
    for T, Hkv, topk in ((4, 1, 17), (512, 1, 17), (64, 8, 32), (1, 1, 1), (1, 1, 3), (1, 1, 1024)):
        n = L.mi_sparse_attention_score_num_chunks(T, Hkv, topk)
        assert 1 <= n <= topk and n & (n - 1) == 0
    run_capi(c, 3)                                             # any count up to topK is served by the C-ABI
    run_capi(c, 6, expect=EINVAL)                              # more chunks than slots
    run_capi(c, 1, expect=EINVAL, sm_scale=0.0)
    run_capi(c, 1, expect=EINVAL, topk=1025)
    run_capi(c, 1, expect=EINVAL, q_stride_h=60)
    run_capi(c, 1, expect=EINVAL, actual_seq_lengths=None)     # tokens != batch
    run_capi(c, 1, expect=EINVAL, q_dequant_scale=f["sq"].data_ptr())
    run_capi(f, 1, expect=EINVAL, v_dequant_scale=None)
    run_capi(f, 1, expect=EINVAL, q_scale_blocks=0)
