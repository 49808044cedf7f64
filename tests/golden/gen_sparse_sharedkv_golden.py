"""Generates tests/golden/sparse_sharedkv_ref_*.npz by running the golden function of the REFERENCE test
(tests/python/sgl_kernel_npu/test_sparse_attn_sharedkv.py of the reference checkout, whose root is the first argument: `_reference_swa`, plain
torch on the CPU).  The function is loaded out of that file by path, with empty stand-ins for the NPU modules the file imports; only the
resulting vectors (small inputs + the golden's output) are committed, the reference source never travels.

`_reference_swa` covers the window part of one sequence without a sink (the reference test switches the sink off with -1e4); the compressed
modes and the sink are pinned by the restatement alone (tests/sparse_sharedkv_ref.py).  To keep each file under the largest fixture already
committed, q and kv sit on a coarse grid (multiples of 1/64 and 1/8: the files compress), rows no token reads hold NaN, and the golden's
fp32 output is stored for every second (S1 = 1) or fourth (S1 = 3) head.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_sparse_sharedkv_golden.py <reference root>
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import sparse_sharedkv_ref as R  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "tests", "python", "sgl_kernel_npu", "test_sparse_attn_sharedkv.py")
    npu = types.ModuleType("torch_npu")
    npu.npu = types.SimpleNamespace(set_device=lambda *a, **k: None, is_available=lambda: False)
    stand_ins = {"sgl_kernel_npu": types.ModuleType("sgl_kernel_npu"), "torch_npu": npu}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("ref_test_sparse_attn_sharedkv", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod._reference_swa


def cases():
    return [
        # a: decode, fp16, pages of 16, the window is the whole prefix
        dict(name="a", dtype=torch.float16, s1=1, L=200, block=16, window=(199, 0)),
        # b: three rows, bf16, pages of 128, window of 5
        dict(name="b", dtype=torch.bfloat16, s1=3, L=203, block=128, window=(5, 0)),
        # c: three rows, fp16, pages of 16, window of 5 reaching forward by 1 (cut by the end of the sequence for the last row)
        dict(name="c", dtype=torch.float16, s1=3, L=198, block=16, window=(5, 1)),
        # d: decode, bf16, pages of 128, the window is the whole prefix
        dict(name="d", dtype=torch.bfloat16, s1=1, L=200, block=128, window=(199, 0)),
    ]


def main():
    golden = load_reference(sys.argv[1])
    for i, cs in enumerate(cases()):
        c = R.make_case("golden_" + cs["name"], "BSND", [cs["L"]], cs["s1"], cs["block"], 0, None, 1, cs["window"], "off", dtype=cs["dtype"],
                        seed=500 + i, grid=(1.0 / 64, 1.0 / 8))
        kv = R.ori_kv(c)
        out = golden(c["q"], kv, c["ori_block_table"], cs["L"], c["softmax_scale"], cs["window"][0], cs["window"][1])
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(c["q"].shape) and not torch.isnan(out).any()
        heads = np.arange(0, R.HEADS, 2 if cs["s1"] == 1 else 4)
        save = dict(dtype=np.array(str(cs["dtype"]).split(".")[1]), q_bits=c["q"].view(torch.int16).numpy(),
                    ori_bits=c["ori_base"].view(torch.int16).numpy(), ori_block=np.int32(cs["block"]),
                    ori_block_table=c["ori_block_table"].numpy(), seqused_kv=c["seqused_kv"].numpy(), softmax_scale=np.float64(c["softmax_scale"]),
                    ori_win_left=np.int32(cs["window"][0]), ori_win_right=np.int32(cs["window"][1]), heads=heads.astype(np.int32),
                    golden=out.numpy()[:, :, heads])
        path = os.path.join(OUT, f"sparse_sharedkv_ref_{cs['name']}.npz")
        np.savez_compressed(path, **save)
        print(cs["name"], "shape", tuple(out.shape), os.path.getsize(path))


if __name__ == "__main__":
    main()
