"""CPU-only: torch.ops.npu.sparse_attn_sharedkv carries the reference's schema; the C-ABI exports its two entries and the workspace query is
host arithmetic; the float64 restatement (tests/sparse_sharedkv_ref.py) reproduces every stored output of the reference test's golden
(tests/golden/sparse_sharedkv_ref_*.npz, written by gen_sparse_sharedkv_golden.py) and satisfies the identities that pin the sink and the
compressed modes; the GPU tests' case table is sharp.  The GPU tests hold the HIP kernel to the same restatement."""
import os
from ctypes import c_int, c_int64, c_size_t

import numpy as np
import pytest
import torch

import sparse_sharedkv_ref as R
from capi import declared_symbols, load

PATHS = R.golden_paths()


def test_op_schema_is_the_reference_schema():
    import sgl_kernel_npu  # noqa: F401

    schema = torch.ops.npu.sparse_attn_sharedkv.default._schema
    text = str(schema)
    # the checks of the reference's test_public_schema_matches_upstream_binding
    assert "ori_kv_stride" not in text and "cmp_kv_stride" not in text
    assert "*" in text
    assert "float softmax_scale=0." in text and "int cmp_ratio=0" in text and "int ori_win_left=128" in text
    # ... and the whole list
    args = [(a.name, str(a.type), a.kwarg_only, a.default_value if a.has_default_value() else "required") for a in schema.arguments]
    opt = [(n, "Optional[Tensor]", True, None) for n in
           ("ori_kv", "cmp_kv", "ori_sparse_indices", "cmp_sparse_indices", "ori_block_table", "cmp_block_table", "cu_seqlens_q",
            "cu_seqlens_ori_kv", "cu_seqlens_cmp_kv", "seqused_q", "seqused_kv", "sinks", "metadata")]
    assert args == [("q", "Tensor", False, "required")] + opt + [
        ("softmax_scale", "float", True, 0.0), ("cmp_ratio", "int", True, 0), ("ori_mask_mode", "int", True, 4), ("cmp_mask_mode", "int", True, 3),
        ("ori_win_left", "int", True, 128), ("ori_win_right", "int", True, 0), ("layout_q", "str", True, "BSND"), ("layout_kv", "str", True, "PA_ND"),
        ("return_softmax_lse", "bool", True, False)]
    assert [str(r.type) for r in schema.returns] == ["Tensor", "Tensor"]


def test_c_abi_entries_are_declared_and_exported_and_the_workspace_query_is_host_arithmetic():
    lib = load("libmi_sgl_kernels.so")
    names = {"mi_sparse_attn_sharedkv_workspace", "mi_sparse_attn_sharedkv"}
    assert names <= set(declared_symbols("mi_sgl_kernels.h"))
    assert all(hasattr(lib, n) for n in names)
    f = lib.mi_sparse_attn_sharedkv_workspace
    f.restype, f.argtypes = c_size_t, [c_int64, c_int64, c_int]
    row = 64 * (512 + 2) * 4                                   # one piece of one token: 64 heads of (O[512], m, l) in fp32
    assert f(7, 1152, 1) == 0                                  # one piece: the kernel writes the output itself
    sizes = [f(7, 1152, n) for n in range(1, 65)]
    assert sizes[1:] == [7 * n * row for n in range(2, 65)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))        # monotone in num_splits
    assert f(7, 1152, 65) == 0 and f(7, 1152, -1) == 0 and f(0, 1152, 2) == 0
    # num_splits = 0: chosen from the rows, the list bound and the CU count (256 when no device answers): one workgroup per CU at least,
    # four tiles of 64 list positions per piece at least, 32 pieces at most
    cus = 256 if not torch.cuda.is_available() else torch.cuda.get_device_properties(0).multi_processor_count

    def chosen(tokens, bound):
        tiles = (bound + 63) // 64
        return max(1, min((cus + tokens - 1) // tokens, max(tiles // 4, 1), 32))

    for tokens, bound in ((1, 1152), (32, 1152), (128, 640), (1, 128 + 1024), (1, 100), (1000, 1152), (1, 1 << 20)):
        n = chosen(tokens, bound)
        assert f(tokens, bound, 0) == (0 if n == 1 else tokens * n * row), (tokens, bound)


def test_the_stored_cases_cover_what_they_must():
    assert len(PATHS) == 4
    seen = set()
    for path in PATHS:
        assert os.path.getsize(path) < 240 * 1000, path
        c = R.load_golden(path)
        L = int(c["seqused_kv"][0])
        assert 195 <= L <= 205
        seen |= {str(c["q"].dtype), f"S1 {c['q'].shape[1]}", f"block {c['ori_block']}", "whole prefix" if c["ori_win_left"] >= L - 1 else "window 5"}
        assert sorted(c["ori_block_table"][0].tolist()) != c["ori_block_table"][0].tolist()      # a shuffled table
    assert seen == {"torch.bfloat16", "torch.float16", "S1 1", "S1 3", "block 16", "block 128", "whole prefix", "window 5"}, seen


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
def test_restatement_reproduces_the_reference_golden(path):
    """_reference_swa is plain softmax in fp32 without P rounding: the restatement is held to it in float64 with P kept exact (the KV dtype
    of the comparison run is float64) and the sink at -1e4, to 1e-6."""
    c = R.load_golden(path)
    exact = dict(c, q=c["q"].double(), ori_base=c["ori_base"].double())
    got = R.attend_ref(exact, round_out=False)[:, :, torch.from_numpy(c["golden_heads"]).long()]
    err = float((got - c["golden"].double()).abs().max())
    print(os.path.basename(path), "max |restatement - golden|", err)
    assert err < 1e-6
    # with P and the output rounded as the kernel does, it stays inside the reference test's own tolerance
    rounded = R.attend_ref(c)[:, :, torch.from_numpy(c["golden_heads"]).long()]
    assert torch.allclose(rounded, c["golden"].double(), rtol=2e-2, atol=2e-2)


def _small(cmp, ratio, K=0, sinks="normal", index_rows=None, seed=7, window=(5, 0)):
    return R.make_case("id", "TND", [1, 77, 300, 131], [1, 2, 3, 1], 16, 32, cmp, ratio, window, sinks, K=K, dtype=torch.bfloat16, seed=seed,
                       index_rows=index_rows)


def test_sinks_far_below_every_score_give_plain_softmax():
    c = _small("dense", 4, sinks="off")
    got = R.attend_ref(c, round_out=False)
    q = c["q"].reshape(-1, R.HEADS, R.D).double()
    for r, (b, i, s1b) in enumerate(R.token_rows(c)):
        lst = R.token_list(c, b, i, s1b)
        if lst is None:
            assert not got.reshape(q.shape)[r].any()
            continue
        kv = torch.cat([R._rows(c["ori_base"], 16, c["ori_block_table"][b], lst[0])] +
                       ([R._rows(c["cmp_base"], 32, c["cmp_block_table"][b], lst[1])] if lst[1] else [])).double()
        x = (q[r] @ kv.T) * (c["softmax_scale"] * R.LOG2E)
        pr = torch.exp2(x - torch.ceil(x.max(dim=1, keepdim=True).values))      # the P rounding wants a whole reference (ref module)
        want = (pr.to(torch.bfloat16).double() @ kv) / pr.sum(dim=1, keepdim=True)
        assert torch.allclose(got.reshape(q.shape)[r], want, rtol=0, atol=1e-12)


def test_indices_listing_every_visible_key_equal_the_dense_form():
    K = 80                                                      # limit reaches 75 here
    every = lambda c, r, limit, K, rng: np.concatenate([rng.permutation(limit), np.full(K - limit, -1)])      # noqa: E731
    sparse = _small("sparse", 4, K=K, index_rows=every)
    dense = dict(sparse, cmp_sparse_indices=None)
    a, b = R.attend_ref(sparse, round_out=False), R.attend_ref(dense, round_out=False)
    assert a.abs().max() > 0.01
    assert torch.allclose(a, b, rtol=0, atol=1e-12)             # the same keys in another order: float64 summation order only


def test_an_all_minus_one_list_equals_no_compressed_cache():
    none = lambda c, r, limit, K, rng: np.full(K, -1)           # noqa: E731
    sparse = _small("sparse", 4, K=8, index_rows=none)
    plain = dict(sparse, cmp_base=None, cmp_sparse_indices=None)
    assert torch.equal(R.attend_ref(sparse), R.attend_ref(plain))
    assert torch.isnan(sparse["cmp_base"]).all()                # nobody reads the compressed cache: all of it is poisoned


@pytest.mark.parametrize("name", sorted(R.SPECS))
def test_case_table_is_sharp(name):
    """Every case has a token whose window is cut by L - 1, one cut by 0, a row of zeros and -- in the compressed cases -- one with
    limit = 0 and (with an index list) one with limit < K; its restatement output holds no NaN although the caches are poisoned."""
    seen, pairs = set(), set()
    for li in range(3):
        c, want = R.case(name, li, torch.bfloat16)
        assert not torch.isnan(want).any()
        assert torch.isnan(c["ori_base"]).any()
        seen |= R.sharpness(c)
        pairs.add((c["ori_block"], c["cmp_block"]))
    need = {"cut by end", "cut by 0", "zero row"}
    if R.SPECS[name][0][0]:
        need |= {"limit 0"}
    if R.SPECS[name][0][0] == "sparse":
        need |= {"limit below K"}
    assert seen >= need, (name, seen)
    assert pairs == set(R.BLOCK_PAIRS)


def test_restatement_in_fp32_stays_far_inside_the_kernel_tolerance():
    """The figure the issue asks to measure before any tolerance is touched: the restatement in fp32 against itself in float64 over the case
    table, both before the output rounding.  It is printed and held to the recorded size (R.MEASURED_FP32_ERROR, within a factor of four
    either way: the order in which torch's float32 kernels sum differs between CPUs); the kernel tolerance stays the issue's, nothing is
    derived from this figure."""
    worst = 0.0
    for name, li in R.VARIANTS:
        c, _ = R.case(name, li, torch.float16)
        worst = max(worst, float((R.attend_ref(c, compute=torch.float32, round_out=False).double() - R.attend_ref(c, round_out=False)).abs().max()))
    print("max |restatement fp32 - float64| over the case table", worst, "recorded", R.MEASURED_FP32_ERROR)
    assert 0.25 * R.MEASURED_FP32_ERROR <= worst <= 4 * R.MEASURED_FP32_ERROR
    assert 8 * R.MEASURED_FP32_ERROR < 1e-3 / 4                # even with the x8 margin for MFMA summation order: well below atol
