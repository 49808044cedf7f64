"""Generates tests/golden/block_score_prefill_ref_fp16_*.npz by running the REFERENCE prefill indexer
(python/sgl_kernel_npu/sgl_kernel_npu/indexer/flash_block_score_prefill.py of the reference checkout, whose root is the first argument) on
the CPU under TRITON_INTERPRET=1.  Only the resulting vectors (inputs + outputs) are committed; the reference source never travels.  fp16
only (the Triton interpreter mishandles bf16).

Each of a-c holds the inputs, the reference's `score` and the reference's `topk_idx`.  The reference's causal mask compares with the PACKED
token index (tests/block_score_prefill_ref.py); `packed_is_true` says whether that is the tokens' true position (one request, no prefix).
For every case the generator tries seeds until, per row and in float64, all gaps among the selected scores and to the best unselected
finite one exceed TOL: the stored order and set are then not a matter of rounding.  d holds a score tensor with exact ties, all -inf rows
and finite blocks behind the causal length, and what flash_prefill_bnsd_topk_from_score makes of it.

    PYTHONDONTWRITEBYTECODE=1 TRITON_INTERPRET=1 python tests/golden/gen_block_score_prefill_golden.py <reference root>
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
from block_score_prefill_ref import NEG, TOL, causal_lens, packed_positions, prefill_scores_ref  # noqa: E402


def load_reference(root):
    base = os.path.join(root, "python", "sgl_kernel_npu", "sgl_kernel_npu", "indexer")
    sys.modules.setdefault("sgl_kernel_npu", types.ModuleType("sgl_kernel_npu"))
    sys.modules.setdefault("sgl_kernel_npu.indexer", types.ModuleType("sgl_kernel_npu.indexer"))
    mods = {}
    for name in ("flash_block_score_decode", "flash_block_score_prefill"):      # the prefill module imports two helpers of the decode one
        spec = importlib.util.spec_from_file_location("sgl_kernel_npu.indexer." + name, os.path.join(base, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["flash_block_score_prefill"]


# requests: (cached prefix, new tokens)
def cases():
    return [
        # a: one request without a prefix -- the packed index IS the position; fused selection
        dict(name="a", H=2, Hkv=2, D=64, bs=16, reqs=[(0, 150)], bsq=8, topk=4, type="max", fused=True, true_lens=True, idt=torch.int32),
        # b: prefixes that cross block boundaries, one token, no token; G = 4; log-sum-exp; int64 tables; torch.topk selection
        dict(name="b", H=4, Hkv=1, D=128, bs=64, reqs=[(70, 40), (130, 1), (50, 0), (100, 60)], bsq=16, topk=2, type="lse", fused=False,
             idt=torch.int64),
        # c: the fused selection with the TRUE causal lengths on packed-convention scores: request 1's tokens 108 .. 127 see block 1 through
        # the leak, which the selection turns into -1 in place; request 0's prefix is hidden and its local block is appended
        dict(name="c", H=1, Hkv=1, D=80, bs=128, reqs=[(130, 20), (0, 140), (50, 30)], bsq=4, topk=2, type="max", fused=True, true_lens=True,
             idt=torch.int32),
    ]


def build(c, seed):
    g = torch.Generator().manual_seed(seed)
    H, Hkv, D, bs = c["H"], c["Hkv"], c["D"], c["bs"]
    lens = [a + b for a, b in c["reqs"]]
    cu = np.concatenate([[0], np.cumsum([b for _, b in c["reqs"]])])
    total_q, n = int(cu[-1]), len(lens)
    mb = -(-max(lens) // bs)
    used = [-(-x // bs) for x in lens]
    pages = sum(used)
    q = torch.randn((total_q, H, D), generator=g).to(torch.float16)
    k = torch.randn((pages, bs, Hkv, D), generator=g).to(torch.float16)
    perm = torch.randperm(pages, generator=g).tolist()
    rtt = torch.zeros((n + 1, mb * bs + 3), dtype=torch.int64)      # requests live in rows 1.. of the map, in reverse order
    pool = torch.tensor([n - r for r in range(n)], dtype=torch.int64)
    for r in range(n):
        for j in range(used[r]):
            rtt[pool[r], j * bs:(j + 1) * bs] = perm.pop() * bs + torch.arange(bs)
    idt = c["idt"]
    return dict(q=q, k=k, cu_seqlens=torch.tensor(cu).to(idt), seq_lens=torch.tensor(lens).to(idt), req_to_token=rtt.to(idt),
                req_pool_indices=pool.to(idt), max_seqlen=max(lens), block_size=bs, block_size_q=c["bsq"], topk=c["topk"], score_type=c["type"],
                sm_scale=float(D) ** -0.5, fused=c["fused"], packed_is_true=len(c["reqs"]) == 1 and c["reqs"][0][0] == 0)


def min_gap(z):
    """Smallest gap among the topk best finite scores of a row and to the best one behind them (float64, packed positions)."""
    sc = prefill_scores_ref(z["q"], z["k"], z["cu_seqlens"], z["seq_lens"], z["req_to_token"], z["req_pool_indices"], z["block_size"],
                            z["max_seqlen"], z["sm_scale"], z["score_type"], query_pos=packed_positions(z["q"].shape[0]))
    gap = np.inf
    for row in sc.reshape(-1, sc.shape[2]):
        top = sorted((x for x in row if x > NEG), reverse=True)[:z["topk"] + 1]
        gap = min([gap] + [a - b for a, b in zip(top, top[1:])])
    return gap


def save(name, z, extra):
    out = {}
    for key, val in {**z, **extra}.items():
        if isinstance(val, torch.Tensor):
            out[key] = val.numpy()
        elif isinstance(val, np.ndarray):
            out[key] = val
        elif isinstance(val, str):
            out[key] = np.array(val)
        elif isinstance(val, bool):
            out[key] = np.int32(val)
        elif isinstance(val, float):
            out[key] = np.float32(val)
        else:
            out[key] = np.int32(val)
    path = os.path.join(OUT, f"block_score_prefill_ref_fp16_{name}.npz")
    np.savez_compressed(path, **out)
    return os.path.getsize(path)


def main():
    mod = load_reference(sys.argv[1])
    for i, c in enumerate(cases()):
        for seed in range(400 + 50 * i, 450 + 50 * i):
            z = build(c, seed)
            gap = min_gap(z)
            if gap > TOL:
                break
        else:
            raise SystemExit(f"case {c['name']}: no seed with gaps above TOL")
        total_q = z["q"].shape[0]
        args = (z["q"], z["k"], z["cu_seqlens"], z["seq_lens"], z["req_to_token"], z["req_pool_indices"], z["block_size_q"], z["block_size"])
        score = mod.flash_prefill_bnsd_score(*args, z["sm_scale"], z["score_type"])
        extra = {}
        pq = None
        if z["fused"]:
            pq = torch.from_numpy(causal_lens(z["cu_seqlens"], z["seq_lens"], total_q))
            extra["per_query_seq_lens"] = pq
        idx = mod.flash_prefill_bnsd_with_topk_idx(*args, z["topk"], z["sm_scale"], z["score_type"], per_query_seq_lens=pq)
        assert idx.dtype == torch.int32 and idx.shape[2] == z["topk"] + int(z["fused"])
        size = save(c["name"], z, dict(extra, score=score.numpy(), topk_idx=idx.numpy()))
        print(c["name"], "seed", seed, "min gap", gap, "score", tuple(score.shape), "idx", tuple(idx.shape), size)

    # d: the selection alone.  Scores from a set of eight values (exact ties), -inf runs, whole -inf rows; lengths from 0 to past the last
    # block, so that finite blocks lie behind the causal length
    g = torch.Generator().manual_seed(77)
    H, T, nblk, topk, bs = 2, 48, 12, 4, 16
    score = (torch.randint(0, 8, (H, T, nblk), generator=g).float() - 3.5) * 0.75
    score[torch.rand((H, T, nblk), generator=g) < 0.3] = float("-inf")
    score[:, ::7] = float("-inf")
    score[0, 1, :] = 1.25                                      # a row of one value: block order
    lens = torch.randint(0, nblk * bs + 6, (T,), generator=g).to(torch.int32)
    lens[:3] = torch.tensor([0, 1, nblk * bs + 40], dtype=torch.int32)
    idx = mod.flash_prefill_bnsd_topk_from_score(score, lens, topk, bs)
    size = save("d", dict(topk=topk, block_size=bs, fused=True), dict(score=score.numpy(), per_query_seq_lens=lens, topk_idx=idx.numpy()))
    print("d", tuple(idx.shape), size)


if __name__ == "__main__":
    main()
