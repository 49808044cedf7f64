"""CPU-only: the float64 restatement of the prefill block-score indexer (tests/block_score_prefill_ref.py) reproduces the stored outputs
of the reference kernels (tests/golden/block_score_prefill_ref_fp16_*.npz: the reference run under the Triton interpreter), the fp32 error
TOL rests on holds on every input of the GPU tests, the case table keeps its ambiguous rows under the cap, and the Python entry points
check their arguments before they reach the device."""
import glob
import os

import numpy as np
import pytest
import torch

import block_score_prefill_ref as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = sorted(glob.glob(os.path.join(GOLD, "block_score_prefill_ref_fp16_*.npz")))
_cache = {}


def scores_of(key, c, query_pos=None, fp32=False, score_type=None):
    """Each restatement is computed once per session and shared."""
    k = (key, None if query_pos is None else "packed", fp32, score_type or c["score_type"])
    if k not in _cache:
        _cache[k] = P.restate(c, query_pos=query_pos, fp32=fp32, score_type=score_type)
    return _cache[k]


def golden(letter):
    path = os.path.join(GOLD, f"block_score_prefill_ref_fp16_{letter}.npz")
    return P.load_golden(path)


def test_the_stored_files_are_present_and_small():
    assert [os.path.basename(p)[-5] for p in PATHS] == ["a", "b", "c", "d"]
    assert all(os.path.getsize(p) < 500_000 for p in PATHS)


@pytest.mark.parametrize("letter", ["a", "b", "c"])
def test_restatement_reproduces_the_reference_kernel(letter):
    c = golden(letter)
    # a: one request without a prefix -- the default (true) positions ARE the packed ones; b, c: the reference's packed convention
    assert c["packed_is_true"] == (letter == "a")
    qp = None if letter == "a" else P.packed_positions(c["total_q"])
    if letter == "a":
        assert np.array_equal(P.true_positions(c["cu_seqlens"], c["seq_lens"], c["total_q"]), P.packed_positions(c["total_q"]))
    sc = scores_of(letter, c, query_pos=qp)
    P.check_scores(c["score"], sc, tol=P.TOL / 2)
    if c["fused"]:
        rows = P.topk_from_score_ref(sc, c["per_query_seq_lens"], c["topk"], c["block_size"])
    else:
        rows = P.select_plain_ref(sc, c["topk"])
    P.check_golden_rows(rows, c)
    if letter == "c":                                           # the case is there for the in-place -1 and the hidden prefix
        w = c["want"][0]
        assert any(w[t, 0] == -1 and w[t, 1] == 0 for t in range(20 + 108, 20 + 128)), "no leaked block was turned into -1 in place"
        assert (w[:20, 2] == 1).all(), "request 0's local block is appended: its prefix is hidden from the packed mask"


def test_the_two_conventions_differ_where_the_issue_says():
    """Request with a prefix: the packed mask hides the prefix; a later request: future keys leak in.  (Stored case c.)"""
    c = golden("c")
    true = scores_of("c", c)
    packed = scores_of("c", c, query_pos=P.packed_positions(c["total_q"]))
    assert (true[0, 0] > P.NEG).tolist() == [True, True] and (packed[0, 0] > P.NEG).tolist() == [True, False]      # prefix 130: block 1 hidden
    t = 20 + 110                                                # request 1, token 110: true position 110, packed index 130
    assert (true[0, t] > P.NEG).tolist() == [True, False] and (packed[0, t] > P.NEG).tolist() == [True, True]


def test_selection_alone_is_reproduced_exactly():
    c = golden("d")
    sc = c["score"]
    assert np.isneginf(sc).all(axis=2).any() and len(np.unique(sc[np.isfinite(sc)])) <= 9       # eight drawn values and the row of 1.25
    rows = P.topk_from_score_ref(sc, c["per_query_seq_lens"], c["topk"], c["block_size"])
    assert np.array_equal(rows, c["want"])
    # the two examples of the specification
    ex = P.topk_from_score_ref(np.array([[[1.0, 5.0, 5.0, 3.0, 9.0]]]), [40], 4, 16)
    assert ex[0, 0].tolist() == [-1, 1, 2, -1, -1]
    ex = P.topk_from_score_ref(np.full((1, 1, 5), P.NEG), [1], 4, 16)
    assert ex[0, 0].tolist() == [-1, -1, -1, -1, 0]


def every_input():
    out = []
    for letter in ("a", "b", "c"):
        c = golden(letter)
        out.append((f"golden_{letter}", c, [c["score_type"]]))
    for case in P.CASES:
        for dt in (torch.bfloat16, torch.float16):
            out.append((f"{case[0]}_{dt}", P.make_case(*case, dt), ["max", "lse"]))
    for i, c in enumerate(P.further_inputs()):
        out.append((f"further_{i}", c, [c["score_type"]]))
    return out


def test_fp32_error_on_every_input_is_within_half_the_tolerance():
    """TOL = 8 x the fp32 error measured for the decode indexer; the same arithmetic here.  A figure above TOL / 2 is a finding to record,
    not a reason to widen TOL."""
    worst = 0.0
    for key, c, types in every_input():
        for st in types:
            f64 = scores_of(key, c, score_type=st)
            f32 = scores_of(key, c, fp32=True, score_type=st)
            fin = f64 > P.NEG
            assert np.array_equal(f32 > P.NEG, fin)
            err = float(np.abs(f32[fin] - f64[fin]).max()) if fin.any() else 0.0
            print(key, st, "max |score_fp32 - score_f64|", err)
            worst = max(worst, err)
    print("worst", worst, "TOL / 2", P.TOL / 2)
    assert worst <= P.TOL / 2, worst


@pytest.mark.parametrize("case", P.CASES, ids=[c[0] for c in P.CASES])
def test_case_table_keeps_its_ambiguous_rows_under_the_cap(case):
    for dt in (torch.bfloat16, torch.float16):
        c = P.make_case(*case, dt)
        assert bool(torch.isnan(c["k_base"]).any())
        lens = P.causal_lens(c["cu_seqlens"], c["seq_lens"], c["total_q"])
        for st in ("max", "lse"):
            sc = scores_of(f"{case[0]}_{dt}", c, score_type=st)
            assert not np.isnan(sc).any(), "the restatement read a masked key"
            assert np.isneginf(sc[:, int(c["cu_seqlens"][-1]):]).all(), "tokens behind cu[n] see nothing"
            P.check_rows(P.select_plain_ref(sc, c["topk"]), sc, c["topk"])
            P.check_rows(P.topk_from_score_ref(sc, lens, c["topk"], c["block_size"]), sc, c["topk"], fused_lens=lens, block_size=c["block_size"])


def test_python_entry_points_check_their_arguments():
    from sgl_kernel_npu.indexer import flash_block_score_prefill as M
    c = P.make_case(*P.CASES[0], torch.float16)
    args = [c["q"], c["k"], c["cu_seqlens"], c["seq_lens"], c["req_to_token"], c["req_pool_indices"], 8, c["block_size"]]
    kw = dict(max_seqlen=c["max_seqlen"])

    def bad(i, val, topk=4, **more):
        a = list(args)
        a[i] = val
        with pytest.raises(AssertionError):
            M.flash_prefill_bnsd_with_topk_idx(*a, topk, c["sm_scale"], **{**kw, **more})

    bad(0, c["q"].float())                                      # dtype
    bad(1, c["k"].to(torch.bfloat16))                           # dtypes differ
    bad(0, c["q"][:, :, :32])                                   # head dims differ
    bad(2, c["cu_seqlens"][:-1])                                # cu_seqlens [n + 1]
    bad(3, c["seq_lens"].float())
    bad(5, c["req_pool_indices"].repeat(2))
    bad(6, 0)                                                   # block_size_q > 0
    bad(7, 32)                                                  # block_size_k is the cache's page size
    bad(0, c["q"], score_type="mean")
    bad(0, c["q"], max_seqlen=16 * 16384 + 1)                   # more than 16384 blocks
    with pytest.raises(AssertionError):
        M.flash_prefill_bnsd_with_topk_idx(*args, 4, 0.0, **kw)                                  # sm_scale > 0
    with pytest.raises(AssertionError):
        M.flash_prefill_bnsd_topk_from_score(torch.zeros((2, 3, 4)), torch.ones(3, dtype=torch.int32), 1025, 16)      # topk <= 1024
    with pytest.raises(AssertionError):
        M.flash_prefill_bnsd_topk_from_score(torch.zeros((2, 3, 4), dtype=torch.float64), torch.ones(3, dtype=torch.int32), 2, 16)
    with pytest.raises(AssertionError):
        M.flash_prefill_bnsd_topk_from_score(torch.zeros((2, 3, 4)), torch.ones(3, dtype=torch.int64), 2, 16)
    with pytest.raises(AssertionError):
        M.flash_prefill_bnsd_topk_from_score(torch.zeros((2, 3, 4)), torch.ones(5, dtype=torch.int32), 2, 16)
    with pytest.raises(AssertionError):
        M.flash_prefill_bnsd_score_attn(*args[:2], c["k"][:-1], *args[2:], c["sm_scale"], **kw)     # V's shape
    assert M.flash_prefill_bnsd_topk_from_score(torch.zeros((2, 3, 4)), torch.ones(3, dtype=torch.int32), 0, 16).shape == (2, 3, 0)
