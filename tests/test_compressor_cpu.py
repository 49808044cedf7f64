"""CPU-only: torch.ops.npu.compressor carries the reference's schema; the C-ABI exports its two entries, the workspace query is host
arithmetic and every refusal of include/mi_sgl_kernels.h comes back from mi_compressor before a pointer is touched (the pointers here are
dummies); the float64 restatement (tests/compressor_ref.py) reproduces every stored result of the reference test's golden
(tests/golden/compressor_ref_*.npz, written by gen_compressor_golden.py) inside the bounds the GPU tests hold the kernel to, with the same fill
mask and the same written state rows, and so does the restatement run in fp32.

Bounds (from the issue, derived there): cmp_kv within 1 ulp of the output dtype taken at max(|ref64|, 2^-6); state rows within
H 2^-24 sum_k |x_k w_k| (+ 2^-24 |ape| on the score half)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import compressor_ref as R
from capi import declared_symbols, load

PATHS = R.golden_paths()
EINVAL = -1


def test_op_schema_is_the_reference_schema():
    import sgl_kernel_npu  # noqa: F401

    schema = torch.ops.npu.compressor.default._schema
    args = [(a.name, str(a.type), a.kwarg_only, a.default_value if a.has_default_value() else "required") for a in schema.arguments]
    req = [(n, "Tensor", False, "required") for n in ("x", "wkv", "wgate", "state_cache", "ape", "norm_weight", "rope_sin", "rope_cos")]
    opt = [(n, "Optional[Tensor]", False, None) for n in ("state_block_table", "cu_seqlens", "seqused", "start_pos")]
    assert args == req + opt + [("rope_head_dim", "int", False, 64), ("cmp_ratio", "int", False, 4), ("coff", "int", False, 1),
                                ("norm_eps", "float", False, 1e-6), ("rotary_mode", "int", False, 1), ("cache_mode", "int", False, 1),
                                ("state_cache_stride_dim0", "int", False, 0)]
    assert [str(r.type) for r in schema.returns] == ["Tensor"]
    assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["state_cache"]


def test_c_abi_entries_are_declared_and_exported_and_the_workspace_query_is_host_arithmetic():
    lib = R.bind(load("libmi_sgl_kernels.so"))
    names = {"mi_compressor_workspace", "mi_compressor"}
    assert names <= set(declared_symbols("mi_sgl_kernels.h"))
    f = lib.mi_compressor_workspace
    cus = 256 if not torch.cuda.is_available() else torch.cuda.get_device_properties(0).multi_processor_count

    def want(T, B, H, D, coff):
        n2 = 2 * coff * D
        tiles = -(-T // 128) * (n2 // (32 if T <= 256 else 128))
        s = 1
        while s < 8 and tiles * s * 2 <= cus and (H // 64) // (s * 2) >= 4:
            s *= 2
        return -(-(B + 1) * 4 // 256) * 256 + s * T * n2 * 4

    for T, B, H, D, coff in ((1, 1, 1024, 512, 2), (128, 128, 4096, 512, 2), (128, 128, 7168, 512, 1), (256, 2, 1024, 128, 2),
                             (257, 2, 1024, 128, 2), (300, 2, 1536, 512, 2), (8192, 1, 4096, 512, 1), (9, 1, 10240, 128, 2)):
        assert f(T, B, H, D, coff) == want(T, B, H, D, coff), (T, B, H, D, coff)
    assert f(0, 1, 1024, 512, 2) == 0 and f(5, 0, 1024, 512, 2) == 0 and f(5, 1, 1000, 512, 2) == 0 and f(5, 1, 512, 512, 2) == 0
    assert f(5, 1, 10752, 512, 2) == 0 and f(5, 1, 1024, 256, 2) == 0 and f(5, 1, 1024, 512, 3) == 0


def test_refusals_come_back_before_a_pointer_is_touched():
    lib = R.bind(load("libmi_sgl_kernels.so"))
    paged = R.make_case("refuse", "c4a", [13], [9], 1)
    ring = R.make_case("refuse", "c4a", [13], [9], 2)
    dummy = {k: 0x10 for k in ("x", "wkv", "wgate", "state_cache", "ape", "norm_weight", "rope_sin", "rope_cos", "state_block_table",
                               "cu_seqlens", "seqused", "start_pos", "cmp_kv", "workspace")}
    ww2 = 2 * paged["coff"] * paged["D"]
    bad = [
        (paged, dict(cmp_ratio=8)), (paged, dict(coff=1)), (paged, dict(head_dim=256)), (paged, dict(cmp_ratio=128)),      # (128, 2, 512)
        (paged, dict(cmp_ratio=128, coff=1, head_dim=128)),
        (paged, dict(hidden=512)), (paged, dict(hidden=10752)), (paged, dict(hidden=1280)),
        (paged, dict(rope_head_dim=32)), (paged, dict(rotary_mode=0)), (paged, dict(rotary_mode=3)), (paged, dict(cache_mode=0)),
        (paged, dict(cache_mode=3)), (paged, dict(dtype=2)), (paged, dict(layout=2)),
        (ring, dict(table_dims=1)), (ring, dict(table_cols=paged["coff"] * paged["r"])),
        (paged, dict(state_cache_stride_dim0=paged["block_size"] * ww2 + 1)), (paged, dict(state_cache_stride_dim0=ww2)),
        (paged, dict(out_rows=R.out_rows(paged) + 1)),
    ]
    for c, over in bad:
        p = R.fill_params(c, dummy, workspace_bytes=1 << 40, **over)
        assert lib.mi_compressor(ctypes.byref(p), None) == EINVAL, over
    # what passes the same checks is refused only for its pointers: the call above never got that far
    assert lib.mi_compressor(ctypes.byref(R.fill_params(paged, dict(dummy, x=0), workspace_bytes=1 << 40)), None) == EINVAL
    assert lib.mi_compressor(ctypes.byref(R.fill_params(paged, dummy, workspace_bytes=16)), None) == EINVAL      # workspace too small
    assert lib.mi_compressor(None, None) == EINVAL
    # the stride may be given: size(1) * size(2)
    ok = R.fill_params(paged, dummy, workspace_bytes=1 << 40, state_cache_stride_dim0=paged["block_size"] * ww2, tokens=0, out_rows=0)
    assert lib.mi_compressor(ctypes.byref(ok), None) == 0                                                      # T = 0: nothing to launch


def test_the_stored_cases_cover_what_they_must():
    assert len(PATHS) == len(R.GOLDEN_CASES) == 8
    seen = set()
    for path in PATHS:
        assert os.path.getsize(path) < 240 * 1000, path
        c, z = R.load_golden(path)
        seen.add((c["shape"], tuple(c["start_pos"].tolist()), c["tokens"], c["cache_mode"]))
        seen.add(str(c["dtype"]))
        assert z["filled"].any() and len(z["state_rows"]) > 0
    assert seen >= {("c4li", (13,), 9, 1), ("c4li", (13,), 9, 2), ("c4a", (13,), 9, 1), ("c4a", (13,), 9, 2), ("c128a", (200,), 129, 1),
                    ("c128a", (200,), 129, 2), ("c128a", (0,), 129, 2), "torch.bfloat16", "torch.float16"}
    assert any(len(c) == 4 and len(c[1]) == 3 for c in seen if isinstance(c, tuple))      # the three-sequence case


@pytest.mark.parametrize("compute", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
def test_restatement_reproduces_the_reference_golden(path, compute):
    """The golden computes in fp32 and rounds once; the restatement (in float64, and again in fp32: the reference arithmetic alone must not
    eat the margin) is held to it by the kernel's own bounds, with the float64 restatement as the value the bounds are taken at."""
    c, z = R.load_golden(path)
    ref64 = R.compress_ref(c, round_out=False)
    got = R.compress_ref(c, compute=compute)
    assert np.array_equal(got["filled"], z["filled"])
    assert np.array_equal(np.flatnonzero(got["written"]), z["state_rows"])
    f = z["filled"]
    golden = torch.from_numpy(z["cmp_kv_bits"]).view(c["dtype"]).double().numpy()
    bound = R.ulp_bound(ref64["cmp_kv"][f], c["dtype"])
    for what, v in (("golden", golden[f]), ("restatement", got["cmp_kv"][f].astype(np.float64))):
        err = np.abs(v - ref64["cmp_kv"][f]) / bound
        print(os.path.basename(path), what, "max |. - ref64| in ulp", float(err.max()))
        assert not np.isnan(v).any() and err.max() <= 1.0
    assert not got["cmp_kv"][~f].any()
    sb = R.state_bound(c, ref64)
    stride = int(z["state_stride"])
    for row, vals in zip(z["state_rows"], z["state_values"]):
        lim = sb[int(row)][::stride]
        for what, v in (("golden", vals.astype(np.float64)), ("restatement", got["state"][row][::stride].astype(np.float64))):
            assert (np.abs(v - ref64["state"][row][::stride]) <= lim).all(), (what, int(row))
