"""GPU parity of the lightning indexer (C-ABI mi_lightning_indexer / mi_lightning_indexer_score and torch.ops.npu.lightning_indexer)
against the float64 restatement (tests/lightning_indexer_ref.py) at the tolerant row check with TOL = 8 x the measured fp32 error, and
against the stored outputs of the reference test's golden.

Every case of the table keeps NaN in the key rows at or behind a sequence's length, in the pages no sequence owns and in a page that every
unused table entry names: a read through such an entry, or of such a row, shows as a wrong row, never as a fault.  Every C-ABI run keeps
sentinels behind the output and the workspace."""
import os
from ctypes import c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import lightning_indexer_ref as R
from capi import load, ptr, stream_ptr

pytestmark = pytest.mark.gpu
EINVAL = -1
DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1}
LQ = {"BSND": 0, "TND": 1}
LK = {"BSND": 0, "TND": 1, "PA_BSND": 2}
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load("libmi_sgl_kernels.so")
        _lib.mi_lightning_indexer_workspace.restype = c_size_t
        _lib.mi_lightning_indexer_workspace.argtypes = [c_int, c_int, c_int, c_int64, c_int64]
        shape = [c_int, c_int, c_int, c_int, c_int64, c_int, c_int, c_int, c_int64, c_int] + [c_int64] * 8
        _lib.mi_lightning_indexer_score.argtypes = [c_void_p] * 4 + [c_int64] + [c_void_p] * 3 + shape + [c_int, c_int, c_void_p]
        _lib.mi_lightning_indexer.argtypes = [c_void_p] * 7 + shape + [c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]
    return _lib


def to_gpu(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def shape_args(c, **over):
    q, k, w = c["query"], c["key"], c["weights"]
    tnd, lk = c["layout_query"] == "TND", c["layout_key"]
    a = dict(lq=LQ[c["layout_query"]], lk=LK[lk], batch=len(c["s2"]), s1=c["S1"], rows=R.num_rows(c), heads=q.shape[-2], key_heads=k.shape[-2],
             head_dim=q.shape[-1], cap=c["capacity"], block_size=k.shape[1] if lk == "PA_BSND" else 0,
             bt_sb=c["block_table"].stride(0) if c["block_table"] is not None else 0, q_s0=q.stride(0), q_s1=0 if tnd else q.stride(1),
             q_sh=q.stride(-2), w_s0=w.stride(0), w_s1=0 if tnd else w.stride(1), k_sblk=0 if lk == "TND" else k.stride(0),
             k_srow=k.stride(0) if lk == "TND" else k.stride(1))
    a.update(over)
    return a, [a[n] for n in ("lq", "lk", "batch", "s1", "rows", "heads", "key_heads", "head_dim", "cap", "block_size", "bt_sb", "q_s0", "q_s1",
                              "q_sh", "w_s0", "w_s1", "k_sblk", "k_srow")]


def run_capi(c, expect=0, count=None, mode=None, dtype=None, drop=(), **over):
    """-> sparse_indices [rows, sparse_count] through mi_lightning_indexer; `over` replaces integer arguments, `drop` names pointers to omit."""
    L = lib()
    a, shape = shape_args(c, **over)
    count = c["sparse_count"] if count is None else count
    wsb = L.mi_lightning_indexer_workspace(LQ[c["layout_query"]], len(c["s2"]), c["S1"], R.num_rows(c), c["capacity"])
    tail = 256
    ws = torch.full((wsb + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    n_out = R.num_rows(c) * max(min(count, R.MAX_SPARSE), 1)
    flat = torch.full((n_out + tail,), -77, dtype=torch.int32, device="cuda")
    pick = lambda name: None if name in drop else ptr(c[name])
    rc = L.mi_lightning_indexer(ptr(c["query"]), ptr(c["key"]), ptr(c["weights"]), ptr(flat), pick("actual_seq_lengths_query"),
                                pick("actual_seq_lengths_key"), pick("block_table"), *shape, count,
                                c["sparse_mode"] if mode is None else mode, DTYPE_CODE[c["query"].dtype] if dtype is None else dtype, ptr(ws),
                                wsb, stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((flat[n_out:] == -77).all()), "wrote behind the output"
    assert bool((ws[wsb:] == 0xA5).all()), "wrote behind the workspace"
    if expect:
        assert bool((flat == -77).all()), "a refused call wrote"
        return None
    return flat[:n_out].view(R.num_rows(c), count)


def run_score(c):
    """-> fp32 scores [rows, ld] through mi_lightning_indexer_score (NaN where the kernel did not write)."""
    _, shape = shape_args(c)
    rows, ld = R.num_rows(c), -(-c["capacity"] // 64) * 64
    tail = 256
    buf = torch.full((rows * ld + tail,), float("nan"), dtype=torch.float32, device="cuda")
    buf[rows * ld:] = 12345.0
    rc = lib().mi_lightning_indexer_score(ptr(c["query"]), ptr(c["key"]), ptr(c["weights"]), ptr(buf), ld, ptr(c["actual_seq_lengths_query"]),
                                          ptr(c["actual_seq_lengths_key"]), ptr(c["block_table"]), *shape, c["sparse_mode"],
                                          DTYPE_CODE[c["query"].dtype], stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((buf[rows * ld:] == 12345.0).all()), "wrote behind the scores"
    return buf[:rows * ld].view(rows, ld)


def run_op(c, sync=True):
    import sgl_kernel_npu  # noqa: F401

    out = torch.ops.npu.lightning_indexer(c["query"], c["key"], c["weights"], actual_seq_lengths_query=c["actual_seq_lengths_query"],
                                          actual_seq_lengths_key=c["actual_seq_lengths_key"], block_table=c["block_table"],
                                          layout_query=c["layout_query"], layout_key=c["layout_key"], sparse_count=c["sparse_count"],
                                          sparse_mode=c["sparse_mode"])
    if sync:
        torch.cuda.synchronize()
    K = c["sparse_count"]
    want = (c["query"].shape[0], 1, K) if c["layout_query"] == "TND" else (c["query"].shape[0], c["query"].shape[1], 1, K)
    assert out.dtype == torch.int32 and tuple(out.shape) == want
    return out.reshape(-1, K)


def check_scores(gpu, scores, visible, tol):
    gpu = gpu.cpu().double().numpy()
    worst = 0.0
    for row, vis in enumerate(visible):
        if vis:
            d = np.abs(gpu[row, :vis] - scores[row][:vis])
            assert not np.isnan(d).any(), f"row {row}: a visible key was not written"
            worst = max(worst, float(d.max()))
    print("max |score_gpu - score_f64| on visible keys", worst, "TOL", tol)
    assert worst <= tol, worst


def check_both(c, ref):
    """Both entries return the same rows; they pass the row check; the scores lie within TOL."""
    idx, scores, visible = ref
    g = to_gpu(c)
    tol = R.TOL[c["family"]]
    a, b = run_capi(g), run_op(g)
    assert torch.equal(a, b), "the C-ABI and the torch op disagree"
    R.check_all(a.cpu().numpy(), scores, visible, c["sparse_count"], tol)
    check_scores(run_score(g), scores, visible, tol)
    return a.cpu().numpy()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", [s[0] for s in R.CASES])
def test_case_table(name, dtype):
    c, ref = R.case(name, dtype)
    check_both(c, ref)


@pytest.mark.parametrize("path", R.golden_paths(), ids=[os.path.basename(p) for p in R.golden_paths()])
def test_stored_golden(path):
    """On the keys a row may see, the kernels return the set the reference test's golden holds (behind them -1, not its masked keys)."""
    c = R.load_golden(path)
    ref = R.indexer_ref(c)
    got = check_both(c, ref)
    gold = c["golden"].reshape(got.shape)
    for row, vis in enumerate(ref[2]):
        n = min(c["sparse_count"], vis)
        assert set(got[row, :n].tolist()) == set(gold[row, :n].tolist())


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["dup", "zero", "neg"])
def test_ties_come_in_ascending_key_order(kind, dtype):
    c = R.tie_case(kind, dtype)
    ref = R.indexer_ref(c)
    got = check_both(c, ref)                                     # check_row holds equal exact scores to ascending keys
    if kind == "zero":
        assert (got == np.arange(c["sparse_count"])[None]).all()
    else:
        s = ref[1][0]
        assert s[got[0, 0]] == s[got[0, 1]] and got[0, 0] + 1 == got[0, 1], "the best score comes twice, the lower key first"
        for row in got:      # sparse_count is odd: a pair is cut at the threshold, behind its lower (even) key, unless the one unpaired key is in
            assert row[-1] % 2 == 0 if 600 not in row.tolist() else (row[-1] % 2 == 1 or row[-1] == 600), row
        assert 600 not in got[0].tolist(), "the first row cuts a pair"
    if kind == "neg":
        assert max(float(s.max()) for s in ref[1]) <= 0.0


@pytest.mark.parametrize("name", ["far_apart", "s2_4100", "bsnd_short_q", "key_bsnd", "key_tnd"])
def test_unused_keys_and_table_entries_do_not_matter(name):
    """NaN in every key row at or behind the lengths, in every page no visible key touches and in the page the unused table entries name:
    the results equal the clean run's bit for bit (indices and visible scores)."""
    dtype = torch.bfloat16
    dirty, ref = R.case(name, dtype)
    clean, _ = R.case(name, dtype, False)
    assert torch.isnan(dirty["key"].float()).any() and not torch.isnan(clean["key"].float()).any()
    gd, gc = to_gpu(dirty), to_gpu(clean)
    assert torch.equal(run_capi(gd), run_capi(gc))
    sd, sc = run_score(gd), run_score(gc)
    for row, vis in enumerate(ref[2]):
        assert torch.equal(sd[row, :vis], sc[row, :vis])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
def test_graph_replay_follows_the_buffers(dtype):
    """Capture once; change query, weights, lengths and table in place; the replay equals an eager call on the new contents."""
    c1, c2 = (to_gpu(c) for c in R.graph_cases(dtype))
    static = dict(c1)
    names = ("query", "weights", "actual_seq_lengths_key", "block_table")
    for n in names:
        static[n] = c1[n].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_op(static, sync=False)                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run_op(static, sync=False)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run_op(c1))
    for n in names:
        static[n].copy_(c2[n])
    graph.replay()
    torch.cuda.synchronize()
    eager = run_op(c2)
    assert torch.equal(out, eager)
    idx, scores, visible = R.indexer_ref(R.graph_cases(dtype)[1])
    R.check_all(eager.cpu().numpy(), scores, visible, c2["sparse_count"], R.TOL["normal"])


def test_row_slices_equal_the_unsliced_run(monkeypatch):
    """MI_LIGHTNING_INDEXER_WS_BYTES lowers the workspace bound: 13 rows in groups of four run as two slices of two groups."""
    c = R.slice_case(torch.bfloat16)
    g = to_gpu(c)
    whole = run_capi(g)
    f = lib().mi_lightning_indexer_workspace
    full = f(1, 2, 1, 13, c["capacity"])
    ld = -(-c["capacity"] // 64) * 64
    assert full == 16 * ld * 4
    monkeypatch.setenv("MI_LIGHTNING_INDEXER_WS_BYTES", str(2 * 4 * ld * 4))
    assert f(1, 2, 1, 13, c["capacity"]) == full // 2
    assert torch.equal(run_capi(g), whole) and torch.equal(run_op(g), whole)
    monkeypatch.setenv("MI_LIGHTNING_INDEXER_WS_BYTES", "1")     # a bound below one group: a group a slice
    assert f(1, 2, 1, 13, c["capacity"]) == full // 4
    assert torch.equal(run_capi(g), whole)
    monkeypatch.delenv("MI_LIGHTNING_INDEXER_WS_BYTES")
    idx, scores, visible = R.indexer_ref(c)
    R.check_all(whole.cpu().numpy(), scores, visible, c["sparse_count"], R.TOL["normal"])


def test_argument_checks_and_limits():
    c = to_gpu(R.case("far_apart", torch.bfloat16)[0])
    b = to_gpu(R.case("key_bsnd", torch.bfloat16)[0])
    # the C-ABI refuses with MI_SGL_EINVAL and writes nothing
    for over in (dict(heads=32), dict(head_dim=64), dict(key_heads=2), dict(dtype=2), dict(count=0), dict(count=2049), dict(mode=1),
                 dict(block_size=24), dict(block_size=2048), dict(cap=R.MAX_KEYS + 16), dict(cap=0), dict(lq=2), dict(lk=3), dict(q_s0=4),
                 dict(drop=("block_table",)), dict(drop=("actual_seq_lengths_query",)), dict(drop=("actual_seq_lengths_key",))):
        run_capi(c, expect=EINVAL, **over)
    run_capi(b, expect=EINVAL, lk=LK["TND"])                       # a non-paged key layout equals the query's
    # the op raises, in the reference's words where the reference checks
    op = torch.ops.npu.lightning_indexer
    q, k, w = c["query"], c["key"], c["weights"]
    kw = dict(actual_seq_lengths_query=c["actual_seq_lengths_query"], actual_seq_lengths_key=c["actual_seq_lengths_key"],
              block_table=c["block_table"], layout_query="TND", layout_key="PA_BSND", sparse_count=16, sparse_mode=3)
    wide = c["block_table"].new_zeros((3, R.MAX_KEYS // 16 + 1))
    bad = [
        (lambda: op(q[:, :32], k, w[:, :32], **kw), "must equal 64"),
        (lambda: op(q[..., :64], k[..., :64], w, **kw), "only support 128"),
        (lambda: op(q, k.half(), w, **kw), "must be the same"),
        (lambda: op(q.float(), k.float(), w.float(), **kw), "float16 or bfloat16"),
        (lambda: op(q, k, w, **dict(kw, sparse_count=0)), "sparse_count must > 0 and <= 2048"),
        (lambda: op(q, k, w, **dict(kw, sparse_count=2049)), "sparse_count must > 0 and <= 2048"),
        (lambda: op(q, k, w, **dict(kw, sparse_mode=1)), "only supported 0 or 3"),
        (lambda: op(q, k.new_zeros((4, 24, 1, 128)), w, **kw), "multiple of 16"),
        (lambda: op(q, k, w, **dict(kw, block_table=None)), "block_table must not be null"),
        (lambda: op(q, k, w, **dict(kw, actual_seq_lengths_query=None)), "actual_seq_lengths_query must not be null"),
        (lambda: op(q, k, w, **dict(kw, actual_seq_lengths_key=None)), "actual_seq_lengths_key must not be null"),
        (lambda: op(q, k, w, **dict(kw, layout_key="BSND")), "should be equal"),
        (lambda: op(q, k, w, **dict(kw, layout_query="SBH")), "only supported BSND or TND"),
        (lambda: op(q, k, w, **dict(kw, block_table=wide)), "keys here"),
    ]
    for i, (call, words) in enumerate(bad):
        with pytest.raises(RuntimeError, match=words):
            call()
            pytest.fail(f"call {i} did not raise")
    # the defaults are the reference's: TND, PA_BSND, 2048, causal
    out = op(q, k, w, actual_seq_lengths_query=c["actual_seq_lengths_query"], actual_seq_lengths_key=c["actual_seq_lengths_key"],
             block_table=c["block_table"])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (q.shape[0], 1, 2048)
    assert torch.equal(out[..., :16].reshape(-1, 16), run_capi(c))      # the order is fixed: the row at sparse_count 16 is a prefix
