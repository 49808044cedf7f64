"""CPU-only: the float64 restatement of the block-score indexer (tests/block_score_ref.py) reproduces every stored output of the reference
kernel (tests/golden/block_score_ref_fp16_*.npz, written by gen_block_score_golden.py); the measured fp32 error behind TOL still holds on
every test input; the GPU tests' case table keeps its ambiguous rows under 2 %; the Python entry points check their arguments.  The GPU
tests hold the HIP kernels to the same restatement."""
import glob
import os

import numpy as np
import pytest
import torch

import block_score_ref as R
from sgl_kernel_npu.indexer import flash_block_score_decode as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = sorted(glob.glob(os.path.join(GOLD, "block_score_ref_fp16_*.npz")))


def restate(c, **over):
    kw = R.ref_kwargs(c)
    kw.update(over)
    return R.block_topk_ref(c["q"], c["k"], c["seq_lens"], c["block_size"], c["max_seqlen"], c["topk"], c["init_blocks"], c["local_blocks"],
                            fused_append_local=c.get("fused", False), max_num_blocks=c["max_num_blocks"], **kw)


def test_the_stored_cases_cover_what_they_must():
    assert len(PATHS) == 5
    seen = set()
    for path in PATHS:
        assert os.path.getsize(path) < 500 * 1000, path
        c = R.load_golden(path)
        topk, bs = c["topk"], c["block_size"]
        assert topk & (topk - 1) == 0, "the reference is right for power-of-two topk only"
        Hq, Hkv, D = c["q"].shape[1], c["k"].shape[2], c["q"].shape[2]
        seen |= {c["score_type"], "hkv1" if Hkv == 1 else "hkv>1", f"block {bs}", f"d {D}", f"forced {c['init_blocks']},{c['local_blocks']}"}
        seen.add("direct" if "req_to_token" in c else "table")
        if "req_to_token" in c and c["req_to_token"].dtype == torch.int64 and c["sanitize"]:
            seen.add("direct int64 sanitised")
        if c["fused"]:
            seen.add("fused append")
        if c["knobs"].get("score_blocks_per_chunk", 16) * 2 <= -(-c["max_seqlen"] // bs):
            seen.add("several score chunks")
        lens = c["seq_lens"].reshape(c["q"].shape[0], -1)
        nbs = -(-lens // bs)
        if c["packed"] and bool(((nbs.max(dim=1).values - nbs.min(dim=1).values) >= 1).any()):
            seen.add("packed rows a block apart")
        if bool((lens % bs != 0).any()):
            seen.add("partly filled last block")
        if bool(((nbs.max(dim=1).values <= topk) & (lens.max(dim=1).values > 0)).any()):
            seen.add("nb <= topk")
        if bool((lens == 0).any()):
            seen.add("len 0")
    assert seen >= {"max", "lse", "hkv1", "hkv>1", "block 16", "block 64", "block 128", "d 64", "d 128", "d 80", "forced 0,0", "forced 1,1",
                    "forced 2,2", "direct", "table", "direct int64 sanitised", "fused append", "several score chunks",
                    "packed rows a block apart", "partly filled last block", "nb <= topk", "len 0"}, seen


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
def test_restatement_reproduces_reference_kernel_outputs(path):
    c = R.load_golden(path)
    idx, scores, scored = restate(c)
    R.check_golden(idx, c)
    # and the stored rows pass the tolerant check against the restatement's scores: they are not a matter of rounding
    assert R.check_all(idx, scores, scored, c["topk"], c["init_blocks"], c["local_blocks"]) == 0


def fp32_error(c):
    worst = 0.0
    for st in ("max", "lse"):
        kw = dict(R.ref_kwargs(c), score_type=st)
        exact = R.block_scores_ref(c["q"], c["k"], c["seq_lens"], c["block_size"], c["max_seqlen"], **kw)
        f32 = R.block_scores_ref(c["q"], c["k"], c["seq_lens"], c["block_size"], c["max_seqlen"], fp32=True, **kw)
        worst = max([worst] + [float(np.abs(x - y).max()) for ra, rb in zip(exact, f32) for x, y in zip(ra, rb) if len(x)])
    return worst


def test_tol_is_eight_times_the_measured_fp32_error_of_every_test_input():
    """TOL is a recorded constant, 8 x the largest fp32 error measured once over every test input.  Re-measured here, the figure is not
    the same on every machine: torch's float32 matmul sums the D products in the order of the BLAS kernel it picks for the CPU and thread
    count at hand, and the largest error over some 1e5 scores is an extreme value that moves with that order (1.23e-6 and 1.38e-6 were
    seen on two x86 machines; a strictly sequential sum of 256 products would lie higher still).  So the re-measured figure must be of
    the recorded size, not equal to it: at most TOL / 2 = 4 x the recorded figure, which still leaves TOL twice above any order's error,
    and at least a quarter of it (a smaller one would mean the measurement no longer measures).  TOL itself does not follow the machine."""
    assert R.TOL == 8 * R.MEASURED_FP32_ERROR
    worst = max([fp32_error(R.load_golden(p)) for p in PATHS] +
                [fp32_error(R.make_case(*case, dtype)) for case in R.CASES for dtype in (torch.bfloat16, torch.float16)] +
                [fp32_error(c) for c in R.further_inputs()])
    print("max |score_fp32 - score_f64| over the test inputs", worst, "recorded", R.MEASURED_FP32_ERROR)
    assert 0.25 * R.MEASURED_FP32_ERROR <= worst <= 4 * R.MEASURED_FP32_ERROR == R.TOL / 2, worst


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_case_table_rows_are_not_ambiguous(case):
    """The restatement's own rows of every GPU case: under 2 % with a boundary gap inside TOL (the share the GPU test allows)."""
    for dtype in (torch.bfloat16, torch.float16):
        c = R.make_case(*case, dtype)
        idx, scores, scored = restate(c)
        R.check_all(idx, scores, scored, c["topk"], c["init_blocks"], c["local_blocks"])
        assert any(any(row) for row in scored), "a case must score something"


def test_further_gpu_inputs_are_not_ambiguous():
    for c in R.further_inputs():
        idx, scores, scored = restate(c)
        assert R.check_all(idx, scores, scored, c["topk"], c["init_blocks"], c["local_blocks"]) == 0


def test_selection_padding_and_forced_blocks():
    nat = [0.5, 3.0, 2.0, 3.0, -1.0]
    assert R.select_ref(nat, 3, 0, 0) == [1, 3, 2]                 # ties by ascending block id
    assert R.select_ref(nat, 8, 0, 0) == [1, 3, 2, 0, 4, -1, -1, -1]   # -1 behind the row's blocks, never a repeat
    assert R.select_ref(nat, 3, 2, 2) == [0, 1, 3]                 # init first (1e30), then local (1e29)
    assert R.select_ref(nat, 4, 4, 4) == [0, 1, 2, 3]              # a block that is init and local ends as local: 0 init, 1 .. 4 local
    assert R.select_ref(list(range(75)), 3, 2, 2) == [0, 1, 73]    # the reference returns [0, 1, 47] here (topk not a power of two)
    out = R.append_local_ref(np.array([[[3, 0, 9, -1], [2, 1, 0, 5]]]), [40, 0], 16, 8)
    assert out.tolist() == [[[-1, 0, -1, -1, 2], [-1, -1, 0, -1, -1]]]


def test_wrapper_argument_checks_raise():
    f = M.flash_decode_bnsd_with_topk_idx
    q = torch.zeros(2, 8, 64, dtype=torch.float16)
    k = torch.zeros(6, 16, 2, 64, dtype=torch.float16)
    bt = torch.zeros(2, 3, dtype=torch.int32)
    lens = torch.tensor([40, 20], dtype=torch.int32)
    rtt = torch.zeros(3, 64, dtype=torch.int32)
    pool = torch.tensor([1, 2], dtype=torch.int32)
    direct = dict(req_to_token=rtt, req_pool_indices=pool, max_num_blocks=3, num_pages=6)
    so = dict(disable_index_value=True)
    bad = [
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0, score_type="mean", **so),
        lambda: f(q.float(), None, k, None, bt, lens, 48, 16, 2, 0, 0, **so),
        lambda: f(q, None, k.to(torch.bfloat16), None, bt, lens, 48, 16, 2, 0, 0, **so),
        lambda: f(q, None, k, None, bt, lens.float(), 48, 16, 2, 0, 0, **so),
        lambda: f(q, None, k, None, None, lens, 48, 16, 2, 0, 0, **so),                              # no page source
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0, **so, **direct),                     # two page sources
        lambda: f(q, None, k, None, None, lens, 48, 16, 2, 0, 0, req_to_token=rtt, **so),           # half a direct map
        lambda: f(q, None, k, None, None, lens, 48, 16, 2, 0, 0, **dict(direct, num_pages=None), **so),
        lambda: f(q, None, k, None, None, lens, 48, 16, 2, 0, 0, **dict(direct, max_num_blocks=5), **so),      # map narrower than the blocks
        lambda: f(q, None, k, k, None, lens, 48, 16, 2, 0, 0, **direct),                            # the direct map is score-only
        lambda: f(q, None, k, None, bt.float(), lens, 48, 16, 2, 0, 0, **so),
        lambda: f(q, None, k, None, bt, lens, 48, 32, 2, 0, 0, **so),                               # block size of the cache
        lambda: f(q, None, k, None, bt, lens[:1], 48, 16, 2, 0, 0, **so),
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0, packed_seq_lens=True, **so),         # packed needs B * G lengths
        lambda: f(q, None, k, k, bt, torch.zeros(8, dtype=torch.int32), 48, 16, 2, 0, 0, packed_seq_lens=True),      # packed is score-only
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0),                                     # the full form needs V
        lambda: f(q, None, k, k[:, :8], bt, lens, 48, 16, 2, 0, 0),
        lambda: f(q, None, k, k, bt, lens, 48, 16, 2, 0, 0, num_kv_chunks=3),                       # not a power of two
        lambda: f(q, None, k, k, bt, lens, 48, 16, 2, 0, 0, num_kv_chunks=0),
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0, fused_append_local=True, **so),      # needs max_num_blocks
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0, runtime_score_short_max_blocks=4, **so),     # both or neither
        lambda: f(q, None, k, None, bt, lens, 48, 16, 2, 0, 0, runtime_score_short_chunks=2, **so),
        lambda: f(q, None, k, None, bt, lens, 16 * 16384 + 1, 16, 2, 0, 0, **so),                   # the declared limits
        lambda: f(q, None, k, None, bt, lens, 48, 16, 1025, 0, 0, **so),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(AssertionError):
            call()
            pytest.fail(f"call {i} did not raise")
    o, idx = f(q, None, k, None, bt, lens, 48, 16, 0, 0, 0, **so)                                   # topk <= 0: empty, nothing launched
    assert o is None and idx.shape == (8, 2, 0) and idx.dtype == torch.int32
    a = M.append_local_block_to_topk_idx
    idx = torch.zeros(2, 2, 4, dtype=torch.int32)
    for call in (lambda: a(idx.long(), lens, 16, 3), lambda: a(idx[:, :, ::2], lens, 16, 3), lambda: a(idx, lens[:1], 16, 3),
                 lambda: a(idx, lens, 0, 3), lambda: a(idx, lens, 16, 0), lambda: a(idx[0], lens, 16, 3)):
        with pytest.raises(AssertionError):
            call()
    n = M._normalize_topk_idx_for_gqa
    per_q = torch.arange(8 * 2 * 3, dtype=torch.int32).reshape(8, 2, 3)
    assert torch.equal(n(per_q, 8, 2, 4), per_q[[0, 4]]) and n(per_q, 8, 2, 4).is_contiguous()
    assert torch.equal(n(per_q[:2], 8, 2, 4), per_q[:2])
    with pytest.raises(AssertionError):
        n(per_q[:3], 8, 2, 4)
    assert [M._floor_power_of_2(x) for x in (0, 1, 2, 3, 4, 7, 8, 1000)] == [1, 1, 2, 2, 4, 4, 8, 512]
