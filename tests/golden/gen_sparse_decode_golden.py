"""Generates tests/golden/gqa_sparse_ref_fp16_*.npz by running the REFERENCE Triton kernel behind
`flash_decode_bnsd_with_gqa_share_sparse` (python/sgl_kernel_npu/sgl_kernel_npu/attention/gqa_share_sparse_attention.py:180-878 of the
reference checkout, whose root is the first argument) on the CPU under TRITON_INTERPRET=1.  Only the resulting vectors (inputs + outputs)
are committed; the reference source never travels.  fp16 only (the Triton interpreter mishandles bf16).  The reference file imports
helpers from its indexer package: both files are loaded by path, with empty parent packages in sys.modules.

    PYTHONDONTWRITEBYTECODE=1 TRITON_INTERPRET=1 python tests/golden/gen_sparse_decode_golden.py <reference root>
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


def load_reference(root):
    pkg = os.path.join(root, "python", "sgl_kernel_npu", "sgl_kernel_npu")
    for name in ("sgl_kernel_npu", "sgl_kernel_npu.indexer"):
        sys.modules.setdefault(name, types.ModuleType(name))

    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    by_path("sgl_kernel_npu.indexer.flash_block_score_decode", os.path.join(pkg, "indexer", "flash_block_score_decode.py"))
    return by_path("ref_gqa_share_sparse_attention", os.path.join(pkg, "attention", "gqa_share_sparse_attention.py"))


# name, B, Hq, Hkv, D, block, max_blocks, seq_lens, chunks, sink, direct-map lookup, per-q-head lists, index dtype, table dtype, lists
# (one list per (kv head or q head, sequence); -1 = hole).  Between them: Hkv of 1 and of more than 1; sink and no sink; holes; a row whose
# list is all -1; the partly filled last block in front of / inside its list; an entry behind the sequence's end; duplicates; direct-map
# lookup; per-q-head lists; blocks of 16 and 64 keys; a head dim that is not a power of two.
def cases():
    c = []
    # a: lens 150 -> blocks 0..9, block 9 holds 6 keys and stands first / in the middle; lens 37 -> blocks 0..2, block 2 holds 5 keys, entry 5
    # lies behind the end
    c.append(dict(name="a", B=2, Hq=8, Hkv=2, D=128, bs=16, max_blocks=10, lens=[150, 37], chunks=2, sink=True, direct=False, per_q=False,
                  idx_dt=torch.int32, tab_dt=torch.int32,
                  lists=[[[9, -1, 3, 0, -1, 7], [2, 5, -1, 0, -1, -1]], [[-1, 4, 9, -1, 1, 8], [-1, -1, 1, 2, 0, -1]]]))
    # b: one kv head, blocks of 64, direct-map lookup with int64 tables, row 1 all -1, no sink, one chunk
    c.append(dict(name="b", B=3, Hq=16, Hkv=1, D=64, bs=64, max_blocks=5, lens=[300, 200, 130], chunks=1, sink=False, direct=True, per_q=False,
                  idx_dt=torch.int64, tab_dt=torch.int64,
                  lists=[[[4, 0, -1, 2, 1], [-1, -1, -1, -1, -1], [-1, 2, -1, -1, 0]]]))
    # c: per-q-head lists (the list of each group's first head counts; the others hold decoys), four chunks, sink, a duplicate
    c.append(dict(name="c", B=2, Hq=8, Hkv=2, D=64, bs=16, max_blocks=8, lens=[128, 99], chunks=4, sink=True, direct=False, per_q=True,
                  idx_dt=torch.int32, tab_dt=torch.int64,
                  lists=[[[7, 2, -1, 2, 5, -1, 0, 3], [6, -1, -1, 1, 0, 4, -1, -1]], [[1, -1, 6, -1, 4, -1, -1, 0], [-1, 6, 3, -1, -1, 5, 2, -1]]]))
    # d: MHA, head dim 80, blocks of 64, direct-map lookup with page sanitising, two chunks, no sink, a duplicate and an entry behind the end
    c.append(dict(name="d", B=2, Hq=2, Hkv=2, D=80, bs=64, max_blocks=3, lens=[140, 64], chunks=2, sink=False, direct=True, per_q=False,
                  idx_dt=torch.int32, tab_dt=torch.int32,
                  lists=[[[2, 0, -1, -1], [0, 0, 1, -1]], [[-1, 2, -1, 1], [-1, -1, -1, -1]]]))
    return c


def main():
    mod = load_reference(sys.argv[1])
    for i, c in enumerate(cases()):
        g = torch.Generator().manual_seed(100 + i)
        B, Hq, Hkv, D, bs, mb = c["B"], c["Hq"], c["Hkv"], c["D"], c["bs"], c["max_blocks"]
        G = Hq // Hkv
        num_pages = B * mb + 2
        q = torch.randn((B, Hq, D), generator=g).to(torch.float16)
        k = torch.randn((num_pages, bs, Hkv, D), generator=g).to(torch.float16)
        v = torch.randn((num_pages, bs, Hkv, D), generator=g).to(torch.float16)
        sink = torch.randn((Hq, D), generator=g).to(torch.float16) if c["sink"] else None
        pages = torch.randperm(num_pages, generator=g)[:B * mb].reshape(B, mb)
        lens = torch.tensor(c["lens"], dtype=torch.int32)
        lists = torch.tensor(c["lists"], dtype=c["idx_dt"])          # [Hkv, B, topk]
        if c["per_q"]:
            full = torch.randint(-1, mb, (Hq, B, lists.shape[2]), generator=g).to(c["idx_dt"])
            full[::G] = lists
            lists = full
        z = dict(q=q.numpy(), k=k.numpy(), v=v.numpy(), topk_idx=lists.numpy(), seq_lens=lens.numpy(), block_size=np.int32(bs),
                 sm_scale=np.float32(D ** -0.5), num_topk_chunks=np.int32(c["chunks"]))
        kw = {}
        if c["direct"]:
            rows = B + 1                                            # requests live in rows 1.. of the map, in reverse order
            rtt = torch.zeros((rows, mb * bs + 3), dtype=c["tab_dt"])
            pool = torch.tensor([rows - 1 - b for b in range(B)], dtype=torch.int32)
            for b in range(B):
                for j in range(mb):
                    rtt[pool[b], j * bs:(j + 1) * bs] = pages[b, j] * bs + torch.arange(bs)
            kw = dict(req_to_token=rtt, req_pool_indices=pool, max_num_blocks=mb, num_pages=num_pages, sanitize_page_ids=c["name"] == "d")
            z.update(req_to_token=rtt.numpy(), req_pool_indices=pool.numpy(), max_num_blocks=np.int32(mb), num_pages=np.int32(num_pages),
                     sanitize_page_ids=np.int32(c["name"] == "d"))
            bt = None
        else:
            bt = pages.to(c["tab_dt"])
            z.update(block_table=bt.numpy())
        if sink is not None:
            z.update(sink=sink.numpy())
        out = mod.flash_decode_bnsd_with_gqa_share_sparse(q, sink, k, v, bt, lens, bs, lists, None, num_topk_chunks=c["chunks"],
                                                          use_native=False, **kw)
        assert not torch.isnan(out.float()).any()
        z.update(out=out.numpy())
        path = os.path.join(OUT, f"gqa_sparse_ref_fp16_{c['name']}.npz")
        np.savez_compressed(path, **z)
        print(c["name"], "ok", float(out.abs().max()), os.path.getsize(path))


if __name__ == "__main__":
    main()
