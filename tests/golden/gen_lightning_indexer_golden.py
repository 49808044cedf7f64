"""Generates tests/golden/lightning_indexer_ref_*.npz by running the golden function of the REFERENCE test
(tests/python/sgl_kernel_npu/test_lightning_indexer.py of the reference checkout, whose root is the first argument: `_lightning_indexer`,
plain torch on the CPU).  The function is loaded out of that file by path, with empty stand-ins for the NPU modules the file imports; only
the resulting vectors (small inputs + the golden's output) are committed, the reference source never travels.

The golden serves paged keys only (layout_key PA_BSND) and, for BSND queries, whole rows (actual_seq_lengths_query = S1).  Case d keeps the
golden's quirk: causal rows that see fewer keys than sparse_count still get min(sparse_count, act_s2) slots, the masked keys among them in
whatever order the sort left them.

For every case the generator tries seeds until, per row and in float64 (tests/lightning_indexer_ref.py), no key other than the n-th best
lies within TOL of it: the stored set is then not a matter of rounding.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_lightning_indexer_golden.py <reference root>
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
import lightning_indexer_ref as R  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "tests", "python", "sgl_kernel_npu", "test_lightning_indexer.py")
    npu = types.ModuleType("torch_npu")
    npu.npu = types.SimpleNamespace(set_device=lambda *a, **k: None)
    utils = types.ModuleType("utils")
    utils.require_npu_op = lambda name: None
    stand_ins = {"sgl_kernel_npu": types.ModuleType("sgl_kernel_npu"), "torch_npu": npu, "torchair": types.ModuleType("torchair"), "utils": utils}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("ref_test_lightning_indexer", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod._lightning_indexer


def cases():
    return [
        # a: TND, causal, bf16, blocks of 16, the reference test's distribution
        dict(name="a", lq="TND", s1=[2, 3], s2=[300, 137], block=16, count=64, mode=3, family="uniform", dtype=torch.bfloat16),
        # b: BSND, every key visible, fp16, blocks of 64
        dict(name="b", lq="BSND", s1=[2, 2], s2=[384, 200], block=64, count=32, mode=0, family="normal", dtype=torch.float16),
        # c: BSND with S1 = 4, causal, bf16, blocks of 128
        dict(name="c", lq="BSND", s1=[4, 4], s2=[384, 130], block=128, count=128, mode=3, family="normal", dtype=torch.bfloat16),
        # d: causal rows that see 36 / 37 / 38 / 39 / 40 keys at sparse_count 38: the golden's quirk in the first two
        dict(name="d", lq="TND", s1=[5], s2=[40], block=16, count=38, mode=3, family="uniform", dtype=torch.float16),
    ]


def main():
    golden = load_reference(sys.argv[1])
    for i, cs in enumerate(cases()):
        for seed in range(100 + 50 * i, 150 + 50 * i):
            c = R.make_case("golden_" + cs["name"], cs["lq"], "PA_BSND", cs["s1"], cs["s2"], cs["block"], cs["count"], cs["mode"],
                            family=cs["family"], seed=seed, poison=False, dtype=cs["dtype"])
            _, scores, visible = R.indexer_ref(c)
            tol = R.TOL[cs["family"]]
            if all(R.free_keys(scores[r], visible[r], cs["count"], tol) == 0 for r in range(len(visible))):
                break
        else:
            raise SystemExit(f"case {cs['name']}: no seed without keys inside TOL of the threshold")
        aq = c["actual_seq_lengths_query"]
        if cs["lq"] == "BSND":
            assert aq is None
            aq_golden = torch.tensor(cs["s1"], dtype=torch.int32)
        else:
            aq_golden = aq
        out = golden(c["query"], c["key"], c["weights"], aq_golden, c["actual_seq_lengths_key"], c["block_table"], cs["lq"], cs["count"],
                     cs["mode"])
        assert out.dtype == torch.int32
        save = dict(layout_query=np.array(cs["lq"]), sparse_count=np.int32(cs["count"]), sparse_mode=np.int32(cs["mode"]),
                    family=np.array(cs["family"]), dtype=np.array(str(cs["dtype"]).split(".")[1]), s1=np.array(cs["s1"], dtype=np.int32),
                    s2=np.array(cs["s2"], dtype=np.int32), S1=np.int32(c["S1"]), query_bits=c["query"].view(torch.int16).numpy(),
                    key_bits=c["key"].view(torch.int16).numpy(), weights_bits=c["weights"].view(torch.int16).numpy(),
                    block_table=c["block_table"].numpy(), actual_seq_lengths_key=c["actual_seq_lengths_key"].numpy(), golden=out.numpy())
        if aq is not None:
            save["actual_seq_lengths_query"] = aq.numpy()
        path = os.path.join(OUT, f"lightning_indexer_ref_{cs['name']}.npz")
        np.savez_compressed(path, **save)
        print(cs["name"], "seed", seed, "shape", tuple(out.shape), os.path.getsize(path))


if __name__ == "__main__":
    main()
