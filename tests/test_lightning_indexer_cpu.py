"""CPU-only: the float64 restatement of the lightning indexer (tests/lightning_indexer_ref.py) reproduces every stored output of the
reference test's golden (tests/golden/lightning_indexer_ref_*.npz, written by gen_lightning_indexer_golden.py) on the keys a row may see;
the measured fp32 error behind TOL still holds on every test input; the GPU tests' case table is sharp (fewer than 1 % of sparse_count keys
of a row lie inside the tolerance window); torch.ops.npu.lightning_indexer carries the reference's schema and the C-ABI exports its three
entries.  The GPU tests hold the HIP kernels to the same restatement."""
import os
from ctypes import c_int, c_int64, c_size_t

import numpy as np
import pytest
import torch

import lightning_indexer_ref as R
from capi import declared_symbols, load

PATHS = R.golden_paths()


def test_the_stored_cases_cover_what_they_must():
    assert len(PATHS) == 4
    seen = set()
    for path in PATHS:
        assert os.path.getsize(path) < 500 * 1000, path
        c = R.load_golden(path)
        seen |= {c["layout_query"], f"mode {c['sparse_mode']}", str(c["query"].dtype), f"block {c['key'].shape[1]}"}
        _, _, visible = R.indexer_ref(c)
        if any(0 < v < c["sparse_count"] for v in visible):
            seen.add("visible below sparse_count")
    assert seen >= {"TND", "BSND", "mode 0", "mode 3", "torch.bfloat16", "torch.float16", "block 16", "block 64", "block 128",
                    "visible below sparse_count"}, seen


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
def test_restatement_reproduces_the_reference_golden(path):
    """As sets on the visible prefix of each row, at the golden's own fp32 error.  Behind the visible prefix the golden holds masked keys
    (its quirk: min(sparse_count, act_s2) slots are filled whatever the row may see); the restatement and the kernels hold -1 there."""
    c = R.load_golden(path)
    K, tol = c["sparse_count"], R.TOL[c["family"]]
    idx, scores, visible = R.indexer_ref(c)
    gold = c["golden"].reshape(len(visible), K)
    quirk = 0
    for row, vis in enumerate(visible):
        n = min(K, vis)
        R.check_row(np.concatenate([gold[row, :n], np.full(K - n, -1, dtype=np.int32)]), scores[row], vis, K, tol)
        assert set(gold[row, :n].tolist()) == set(idx[row, :n].tolist())      # the generator kept every window empty
        filled = min(K, len(scores[row]))
        assert (gold[row, n:filled] >= vis).all() and (gold[row, filled:] == -1).all()
        quirk += filled - n
    if path.endswith("_d.npz"):
        assert quirk == 3, "case d shows the golden's masked keys: rows that see 36 and 37 keys at sparse_count 38"


def all_inputs():
    for spec in R.CASES:
        for dtype in R.DTYPES:
            yield R.case(spec[0], dtype)
    for c in R.further_inputs():
        yield c, R.indexer_ref(c)
    for p in PATHS:
        c = R.load_golden(p)
        yield c, R.indexer_ref(c)


def test_tol_is_eight_times_the_measured_fp32_error_of_every_test_input():
    """TOL[family] is a recorded constant, 8 x the largest fp32 error measured once over every test input of the family.  Re-measured here
    the figure moves with the order in which torch's float32 kernels sum on the CPU at hand, so it must be of the recorded size, not equal
    to it: at most TOL / 2 = 4 x the record, at least a quarter of it (test_block_score_cpu.py has the reasoning)."""
    worst = {f: 0.0 for f in R.TOL}
    for c, (_, s64, _) in all_inputs():
        _, s32, _ = R.indexer_ref(c, fp32=True)
        worst[c["family"]] = max([worst[c["family"]]] + [float(np.abs(a - b).max()) for a, b in zip(s64, s32) if a is not None and len(a)])
    for f, rec in R.MEASURED_FP32_ERROR.items():
        print("family", f, "max |score_fp32 - score_f64|", worst[f], "recorded", rec)
        assert R.TOL[f] == 8 * rec
        assert 0.25 * rec <= worst[f] <= 4 * rec == R.TOL[f] / 2, (f, worst[f])


@pytest.mark.parametrize("name", [s[0] for s in R.CASES])
def test_case_table_is_sharp(name):
    """Per row, fewer than 1 % of sparse_count keys besides the n-th best lie inside [s_n - TOL, s_n + TOL]; the restatement's own rows
    pass the row check."""
    for dtype in R.DTYPES:
        c, (idx, scores, visible) = R.case(name, dtype)
        tol, K = R.TOL[c["family"]], c["sparse_count"]
        R.check_all(idx, scores, visible, K, tol)
        free = [R.free_keys(scores[r], v, K, tol) for r, v in enumerate(visible) if v]
        print(name, dtype, "free keys per row", free)
        assert all(f < 0.01 * K for f in free), free


def test_check_row_catches_what_it_must():
    s = np.array([0.5, 3.0, 2.0, 3.0, -1.0, -0.0, 0.0])
    assert R.select_ref(s, 7, 3).tolist() == [1, 3, 2]                              # ties by ascending key
    assert R.select_ref(s, 7, 9).tolist() == [1, 3, 2, 0, 5, 6, 4, -1, -1]          # -0.0 == +0.0; -1 behind the visible keys
    assert R.select_ref(s, 2, 3).tolist() == [1, 0, -1]                             # never a key the row must not see
    R.check_row([1, 3, 2], s, 7, 3, 1e-9)
    for bad in ([3, 1, 2], [1, 3, 0], [1, 1, 2], [1, 3, -1], [1, 2, 3], [1, 3, 7]):
        with pytest.raises(AssertionError):
            R.check_row(bad, s, 7, 3, 1e-9)
    with pytest.raises(AssertionError):
        R.check_row([1, 0, 2], s, 2, 3, 1e-9)                                       # an entry behind n = 2
    assert [R.visible_count(3, 5, 3, r) for r in range(5)] == [0, 0, 1, 2, 3]
    assert [R.visible_count(0, 5, 3, r) for r in range(5)] == [3] * 5


def test_op_schema_is_the_reference_schema():
    import sgl_kernel_npu  # noqa: F401

    schema = torch.ops.npu.lightning_indexer.default._schema
    args = [(a.name, str(a.type), a.default_value if a.has_default_value() else "required") for a in schema.arguments]
    assert args == [("query", "Tensor", "required"), ("key", "Tensor", "required"), ("weights", "Tensor", "required"),
                    ("actual_seq_lengths_query", "Optional[Tensor]", None), ("actual_seq_lengths_key", "Optional[Tensor]", None),
                    ("block_table", "Optional[Tensor]", None), ("layout_query", "Optional[str]", None), ("layout_key", "Optional[str]", None),
                    ("sparse_count", "Optional[int]", None), ("sparse_mode", "Optional[int]", None)]
    assert [str(r.type) for r in schema.returns] == ["Tensor"]


def test_c_abi_entries_are_declared_and_exported():
    lib = load("libmi_sgl_kernels.so")
    names = {"mi_lightning_indexer_workspace", "mi_lightning_indexer_score", "mi_lightning_indexer"}
    assert names <= set(declared_symbols("mi_sgl_kernels.h"))
    assert all(hasattr(lib, n) for n in names)
    # the workspace query is host arithmetic: rows x capacity rounded up to 64 x 4 bytes, rows in whole groups of four unless no sequence
    # can hold two; 0 beyond the declared limit
    f = lib.mi_lightning_indexer_workspace
    f.restype, f.argtypes = c_size_t, [c_int, c_int, c_int, c_int64, c_int64]
    assert f(1, 3, 1, 3, 100) == 3 * 128 * 4                   # TND decode: one row a group
    assert f(1, 2, 1, 5, 100) == 8 * 128 * 4                   # TND, two groups of four rows
    assert f(0, 2, 2, 4, 64) == 2 * 4 * 64 * 4                 # BSND, S1 = 2: a group of four per sequence
    assert f(0, 1, 1, 1, R.MAX_KEYS) == R.MAX_KEYS * 4 and f(0, 1, 1, 1, R.MAX_KEYS + 1) == 0
    assert f(1, 4096, 1, 8192, 65536) == 256 << 20             # larger inputs run in slices of rows under the 256 MiB bound
