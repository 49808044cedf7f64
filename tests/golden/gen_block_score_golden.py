"""Generates tests/golden/block_score_ref_fp16_*.npz by running the REFERENCE `flash_decode_bnsd_with_topk_idx` (score-only form,
python/sgl_kernel_npu/sgl_kernel_npu/indexer/flash_block_score_decode.py of the reference checkout, whose root is the first argument) on
the CPU under TRITON_INTERPRET=1.  Only the resulting vectors (inputs + outputs) are committed; the reference source never travels.  fp16
only (the Triton interpreter mishandles bf16); topk a power of two only (the reference's per-chunk top-k is wrong otherwise).
The sequences of a case draw their pages from one shared pool, which keeps the files small.

For every case the generator tries seeds until, per row and in float64 (tests/block_score_ref.py), all pairwise gaps among the selected
natural scores and the gap to the best unselected one exceed TOL: the stored order and set are then not a matter of rounding.

    PYTHONDONTWRITEBYTECODE=1 TRITON_INTERPRET=1 python tests/golden/gen_block_score_golden.py <reference root>
"""
import importlib.util
import os
import sys
import types

os.environ["TRITON_INTERPRET"] = "1"
sys.dont_write_bytecode = True
import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from block_score_ref import TOL, block_topk_ref, forced_scores  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "python", "sgl_kernel_npu", "sgl_kernel_npu", "indexer", "flash_block_score_decode.py")
    sys.modules.setdefault("sgl_kernel_npu", types.ModuleType("sgl_kernel_npu"))      # the module probes for a native op: none here
    spec = importlib.util.spec_from_file_location("ref_flash_block_score_decode", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


# lens: per sequence, or per row of the group (packed).  pool: pages the sequences share.
def cases():
    return [
        # a: several kv heads, blocks of 16, no forced blocks, several score chunks; a partly filled last block, a sequence with nb <= topk,
        # an empty one
        dict(name="a", B=4, Hq=8, Hkv=2, D=64, bs=16, pool=76, lens=[75 * 16 - 5, 40 * 16, 5 * 16, 0], topk=8, init=0, local=0, type="max",
             tab_dt=torch.int32, len_dt=torch.int32, knobs=dict(score_blocks_per_chunk=4)),
        # b: one kv head, head dim 80, blocks of 64, log-sum-exp scores, direct-map lookup with int64 tables and sanitising
        dict(name="b", B=2, Hq=16, Hkv=1, D=80, bs=64, pool=41, lens=[40 * 64 - 30, 33 * 64 + 1], topk=4, init=1, local=1, type="lse",
             tab_dt=torch.int64, len_dt=torch.int64, direct=True, sanitize=True, knobs=dict()),
        # c: blocks of 128, two forced blocks at either end, the fused causal-local append; a sequence with nb <= topk
        dict(name="c", B=3, Hq=4, Hkv=1, D=64, bs=128, pool=20, lens=[20 * 128 - 17, 11 * 128 + 1, 3 * 128], topk=8, init=2, local=2, type="max",
             tab_dt=torch.int32, len_dt=torch.int32, fused=True, knobs=dict()),
        # d: packed lengths, the rows of a group one block apart (and a group whose rows hold topk and topk + 1 blocks), head dim 128
        dict(name="d", B=3, Hq=4, Hkv=1, D=128, bs=16, pool=66, lens=[1000, 1016, 1032, 1048, 300, 316, 284, 300, 128, 128, 144, 129], topk=8,
             init=0, local=0, type="lse", tab_dt=torch.int32, len_dt=torch.int32, packed=True, knobs=dict(score_blocks_per_chunk=8)),
        # e: many small score chunks, (1, 1) forced blocks; nb <= topk and an empty sequence
        dict(name="e", B=3, Hq=4, Hkv=2, D=64, bs=64, pool=24, lens=[24 * 64 - 55, 100, 0], topk=4, init=1, local=1, type="max",
             tab_dt=torch.int64, len_dt=torch.int32, knobs=dict(score_blocks_per_chunk=2, score_max_chunks=64)),
    ]


def build(c, seed):
    g = torch.Generator().manual_seed(seed)
    B, Hq, Hkv, D, bs, pool = c["B"], c["Hq"], c["Hkv"], c["D"], c["bs"], c["pool"]
    G = Hq // Hkv
    packed = c.get("packed", False)
    lens = torch.tensor(c["lens"], dtype=c["len_dt"])
    per_seq = lens.reshape(B, G).max(dim=1).values if packed else lens
    max_seqlen = int(per_seq.max())
    mb = -(-max_seqlen // bs)
    assert mb <= pool
    q = torch.randn((B, Hq, D), generator=g).to(torch.float16)
    k = torch.randn((pool, bs, Hkv, D), generator=g).to(torch.float16)
    table = torch.stack([torch.randperm(pool, generator=g)[:mb] for _ in range(B)])
    z = dict(q=q, k=k, seq_lens=lens, max_seqlen=max_seqlen, block_size=bs, topk=c["topk"], init_blocks=c["init"], local_blocks=c["local"],
             score_type=c["type"], sm_scale=float(D) ** -0.5, packed=packed, max_num_blocks=mb, fused=c.get("fused", False), knobs=c["knobs"])
    if c.get("direct"):
        rows = B + 1                                            # requests live in rows 1.. of the map, in reverse order
        rtt = torch.zeros((rows, mb * bs + 3), dtype=c["tab_dt"])
        pool_idx = torch.tensor([rows - 1 - b for b in range(B)], dtype=c["tab_dt"])
        for b in range(B):
            for j in range(mb):
                rtt[pool_idx[b], j * bs:(j + 1) * bs] = table[b, j] * bs + torch.arange(bs)
        z.update(req_to_token=rtt, req_pool_indices=pool_idx, num_pages=pool, sanitize=c.get("sanitize", False))
    else:
        z["block_table"] = table.to(c["tab_dt"])
    return z


def ref_kw(z):
    kw = dict(sm_scale=z["sm_scale"], score_type=z["score_type"], packed_seq_lens=z["packed"])
    if "req_to_token" in z:
        kw.update(req_to_token=z["req_to_token"], req_pool_indices=z["req_pool_indices"], num_pages=z["num_pages"], sanitize_page_ids=z["sanitize"])
    else:
        kw.update(block_table=z["block_table"])
    return kw


def min_gap(z):
    """Smallest gap, over the rows that are scored, among the selected natural scores and to the best unselected one (float64)."""
    idx, scores, scored = block_topk_ref(z["q"], z["k"], z["seq_lens"], z["block_size"], z["max_seqlen"], z["topk"], z["init_blocks"],
                                         z["local_blocks"], **ref_kw(z))
    gap = np.inf
    for b, rows in enumerate(scores):
        for h, nat in enumerate(rows):
            if not scored[b][h] or len(nat) == 0:
                continue
            forced = forced_scores(nat, z["init_blocks"], z["local_blocks"])
            natural = sorted((nat[j] for j in range(len(nat)) if forced[j] < 1e28), reverse=True)
            kn = sum(1 for j in idx[h, b] if j >= 0 and forced[j] < 1e28)
            top = natural[:kn + 1]                              # the selected ones and the best one left out
            gap = min([gap] + [a - b_ for a, b_ in zip(top, top[1:])])
    return gap


def main():
    mod = load_reference(sys.argv[1])
    for i, c in enumerate(cases()):
        for seed in range(200 + 50 * i, 250 + 50 * i):
            z = build(c, seed)
            gap = min_gap(z)
            if gap > TOL:
                break
        else:
            raise SystemExit(f"case {c['name']}: no seed with gaps above TOL")
        direct = "req_to_token" in z
        kw = dict(z["knobs"])
        if direct:
            kw.update(req_to_token=z["req_to_token"], req_pool_indices=z["req_pool_indices"], num_pages=z["num_pages"],
                      sanitize_page_ids=z["sanitize"])
        if direct or z["fused"]:
            kw.update(max_num_blocks=z["max_num_blocks"])
        o, out = mod.flash_decode_bnsd_with_topk_idx(
            z["q"], None, z["k"], None, z.get("block_table"), z["seq_lens"], z["max_seqlen"], z["block_size"], z["topk"], z["init_blocks"],
            z["local_blocks"], z["sm_scale"], z["score_type"], disable_index_value=True, packed_seq_lens=z["packed"],
            fused_append_local=z["fused"], use_native=False, **kw)
        assert o is None and out.dtype == torch.int32
        save = {}
        for key, val in z.items():
            if key == "knobs":
                for kk, vv in val.items():
                    save["knob_" + kk] = np.int32(vv)
            elif isinstance(val, torch.Tensor):
                save[key] = val.numpy()
            elif isinstance(val, str):
                save[key] = np.array(val)
            elif isinstance(val, bool):
                save[key] = np.int32(val)
            elif isinstance(val, float):
                save[key] = np.float32(val)
            else:
                save[key] = np.int32(val)
        save["topk_idx"] = out.numpy()
        path = os.path.join(OUT, f"block_score_ref_fp16_{c['name']}.npz")
        np.savez_compressed(path, **save)
        print(c["name"], "seed", seed, "min gap", gap, "shape", tuple(out.shape), os.path.getsize(path))


if __name__ == "__main__":
    main()
