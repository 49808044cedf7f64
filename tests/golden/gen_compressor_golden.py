"""Generates tests/golden/compressor_ref_*.npz by running the golden function of the REFERENCE test (tests/python/sgl_kernel_npu/
test_compressor.py of the reference checkout, whose root is the first argument: `_reference_compressor`, plain numpy in fp32 on the CPU).  The
function is loaded out of that file by path, with empty stand-ins for the NPU modules the file imports; only recorded results are committed,
the reference source never travels.

The inputs are NOT stored: a case is rebuilt from its seed and parameters by tests/compressor_ref.py (every input is an integer draw on a
grid bf16 and fp16 hold exactly), and a crc32 of every rebuilt input is stored to prove it.  Stored per case: the spec, the checksums, the
golden's cmp_kv (bits of the case's dtype) and its fill mask, and the state rows the golden wrote (flat row numbers, and their values at every
`stride`-th channel, the stride chosen so that a file stays under 240 kB).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_compressor_golden.py <reference root>
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import compressor_ref as R  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "tests", "python", "sgl_kernel_npu", "test_compressor.py")
    npu = types.ModuleType("torch_npu")
    npu.npu = types.SimpleNamespace(set_device=lambda *a, **k: None, is_available=lambda: False)
    stand_ins = {"sgl_kernel_npu": types.ModuleType("sgl_kernel_npu"), "torch_npu": npu}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("ref_test_compressor", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod._reference_compressor


def main():
    golden = load_reference(sys.argv[1])
    for spec in R.GOLDEN_CASES:
        c = R.golden_case(spec)
        ww = c["coff"] * c["D"]
        kv_state, score_state = c["state_cache"][..., :ww].clone(), c["state_cache"][..., ww:].clone()
        upd_kv, upd_score = torch.zeros_like(kv_state, dtype=torch.bool), torch.zeros_like(score_state, dtype=torch.bool)
        with np.errstate(invalid="ignore"):
            out, mask = golden(c["x"], c["wkv"], c["wgate"], kv_state, score_state, upd_kv, upd_score, c["ape"], c["norm_weight"], c["rope_sin"],
                               c["rope_cos"], block_table=c["state_block_table"], cu_seqlens=c["cu_seqlens"].tolist(), seqused=c["spans"],
                               start_pos=c["start_pos"].tolist(), rope_head_dim=64, cmp_ratio=c["r"], coff=c["coff"], norm_eps=c["norm_eps"],
                               rotary_mode=c["rotary_mode"], cache_mode=c["cache_mode"])
        assert out.dtype == c["dtype"] and tuple(out.shape) == (R.out_rows(c), c["D"])
        mask = np.asarray(mask)
        assert (mask.all(axis=1) == mask.any(axis=1)).all()
        filled = mask.all(axis=1)
        assert not torch.isnan(out.float()[torch.from_numpy(filled)]).any()
        wrote = upd_kv.view(-1, ww).numpy()
        assert (wrote.all(axis=1) == wrote.any(axis=1)).all() and np.array_equal(wrote, upd_score.view(-1, ww).numpy())
        rows = np.flatnonzero(wrote.all(axis=1)).astype(np.int32)
        stride = 1
        while len(rows) * (2 * ww // stride) * 4 > 200 * 1000:
            stride *= 2
        state = torch.cat([kv_state, score_state], dim=2).view(-1, 2 * ww).numpy()[rows][:, ::stride]
        path = os.path.join(OUT, f"compressor_ref_{spec['name']}.npz")
        np.savez_compressed(path, spec=np.array(json.dumps(spec, sort_keys=True)), checksums=R.checksums(c),
                            cmp_kv_bits=out.view(torch.int16).numpy(), filled=filled, state_rows=rows, state_stride=np.int32(stride),
                            state_values=state.astype(np.float32))
        print(spec["name"], "out", tuple(out.shape), "filled", int(filled.sum()), "state rows", len(rows), "stride", stride, os.path.getsize(path))


if __name__ == "__main__":
    main()
