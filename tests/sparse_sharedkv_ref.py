"""float64 restatement of sparse_attn_sharedkv (include/mi_sgl_kernels.h) and the case builder of its tests.

Per token i of sequence b, L = seqused_kv[b], p = L - S1_b + i (p < 0 or L <= 0: zeros): window keys n in [max(p - left, 0), min(p + right,
L - 1)] of ori_kv, plus -- with cmp_kv -- limit = (p + 1) // cmp_ratio and either the keys j < limit of cmp_kv or every index slot with
0 <= idx < limit (each slot judged on its own, a duplicate counts twice).  s = (q . k) * scale; one softmax over both parts with a virtual key
of logit sinks[h] (not scaled) and value 0; P is rounded to the KV dtype before P.V while the denominator sums the unrounded P (the kernel's
convention, as in the MLA decode golden); the output is rounded once.  P is formed against a reference that is a whole number in the log2
domain, P = 2^(x - M) with x = s log2(e) and M = ceil(max(x, sink log2(e))): another whole M scales P by a power of two, which the rounding
commutes with, so the rounded P -- unlike one formed against the running maximum itself -- does not depend on the order in which a kernel
meets the keys, on its split count or on where its reference starts (the sink).  That matters for rows of a few keys: their output is a sum
of terms of either sign, and the rounding error of each P is relative to its term, not to the sum.

Every row and page no token may read holds NaN: rows of a visible page outside every token's list, pages no table names, and one page that
every unused table entry names.  The caches are stored as [pages, stride] with stride > block * 512 (a strided page dimension)."""
import glob
import os

import numpy as np
import torch

HEADS, D = 64, 512
SCALE = 512 ** -0.5
LOG2E = 1.4426950408889634
DTYPES = (torch.bfloat16, torch.float16)
LENS = (1, 3, 127, 128, 129, 255, 256, 257, 640, 1500)
BLOCK_PAIRS = ((16, 128), (128, 16), (64, 64))
PAD = 64      # elements between the end of a page's rows and the next page

# Measured once, should the kernel tolerance of the issue (atol 1e-3, rtol 2^-7 / 2^-10) ever not hold for a correct kernel: the largest
# |restatement in fp32 - restatement in float64| over the case table, before the output rounding (test_sparse_sharedkv_cpu.py re-measures and
# prints it).  It is a P that rounds the other way in a window of six keys, not summation error.  Not used to widen anything.
MEASURED_FP32_ERROR = 2.0e-5


def tol(dtype):
    return dict(atol=1e-3, rtol=2 ** -7 if dtype == torch.bfloat16 else 2 ** -10)


def paged_view(base, block):
    """[pages, stride] storage -> the [pages, block, 1, 512] cache view with a strided page dimension."""
    return base[:, :block * D].view(base.shape[0], block, 1, D)


def token_rows(c):
    """(b, i, S1_b) of every query row in storage order; rows that belong to no sequence carry b = -1."""
    if c["layout_q"] == "TND":
        cu = c["cu_seqlens_q"].tolist()
        rows = [(-1, 0, 0)] * c["q"].shape[0]
        for b in range(len(cu) - 1):
            for i in range(cu[b + 1] - cu[b]):
                rows[cu[b] + i] = (b, i, cu[b + 1] - cu[b])
        return rows
    B, S1 = c["q"].shape[:2]
    sq = c["seqused_q"].tolist() if c.get("seqused_q") is not None else [S1] * B
    return [(b, i, min(max(sq[b], 0), S1)) for b in range(B) for i in range(S1)]


def token_list(c, b, i, s1b, idx_row=None):
    """-> (window keys, compressed keys that count (with repeats), limit) of one token, or None for a row of zeros."""
    L = int(c["seqused_kv"][b]) if b >= 0 else 0
    p = L - s1b + i
    if b < 0 or i >= s1b or p < 0 or L <= 0:
        return None
    win = list(range(max(p - c["ori_win_left"], 0), min(p + c["ori_win_right"], L - 1) + 1))
    if c.get("cmp_base") is None:
        return win, [], 0
    limit = (p + 1) // c["cmp_ratio"]
    if idx_row is None:
        return win, list(range(limit)), limit
    return win, [int(j) for j in idx_row if 0 <= int(j) < limit], limit


def _rows(base, block, table_row, keys):
    kv = paged_view(base, block)
    pages = table_row[torch.tensor([k // block for k in keys], dtype=torch.long)].long()
    return kv[pages, torch.tensor([k % block for k in keys], dtype=torch.long), 0]


def attend_ref(c, compute=torch.float64, indices="own", round_out=True):
    """-> out [rows, 64, 512] in `compute` precision, rounded once to the case's dtype (and back) unless round_out is off."""
    dtype = c["q"].dtype
    q = c["q"].reshape(-1, HEADS, D)
    idx = c.get("cmp_sparse_indices") if indices == "own" else indices
    idx = None if idx is None else idx.reshape(q.shape[0], -1)
    sink = c["sinks"].to(compute)
    out = torch.zeros(q.shape, dtype=compute)
    for r, (b, i, s1b) in enumerate(token_rows(c)):
        lst = token_list(c, b, i, s1b, None if idx is None else idx[r].tolist())
        if lst is None:
            continue
        win, cmp, _ = lst
        kv = _rows(c["ori_base"], c["ori_block"], c["ori_block_table"][b], win)
        if cmp:
            kv = torch.cat([kv, _rows(c["cmp_base"], c["cmp_block"], c["cmp_block_table"][b], cmp)])
        kv = kv.to(compute)
        assert not torch.isnan(kv).any(), "the restatement read a poisoned row"
        x = (q[r].to(compute) @ kv.T) * (c["softmax_scale"] * LOG2E)
        m = torch.ceil(torch.maximum(x.max(dim=1).values, sink * LOG2E))
        pr = torch.exp2(x - m[:, None])
        l = pr.sum(dim=1) + torch.exp2(sink * LOG2E - m)
        out[r] = (pr.to(dtype).to(compute) @ kv) / l[:, None]
    return (out.to(dtype).to(compute) if round_out else out).reshape(c["q"].shape)


def _grid(x, step):
    return np.round(x / step) * step if step else x


def _paged(rng, lens_keys, block, used, dtype, step=0.0):
    """A poisoned cache for sequences of lens_keys[b] keys of which only used[b] (a set) may be read -> (base, table)."""
    need = [(n + block - 1) // block for n in lens_keys]
    cols = max(need + [1]) + 1
    pages = sum(need) + 2                                   # + the page every unused entry names + a page no table names
    order = rng.permutation(pages)
    trap, ids = int(order[0]), order[2:]
    table = torch.full((len(lens_keys), cols), trap, dtype=torch.int32)
    base = torch.full((pages, block * D + PAD), float("nan"), dtype=dtype)
    kv = paged_view(base, block)
    at = 0
    for b, n in enumerate(need):
        for pg in range(n):
            table[b, pg] = int(ids[at + pg])
        for k in sorted(used[b]):
            kv[int(ids[at + k // block]), k % block, 0] = torch.from_numpy(_grid(0.5 * rng.standard_normal(D), step).astype(np.float32)).to(dtype)
        at += n
    return base, table


def make_case(name, layout, lens, s1, ori_block, cmp_block, cmp, ratio, window, sinks, K=0, dtype=torch.bfloat16, seed=0, seqused_q=None,
              index_rows=None, grid=(0.0, 0.0)):
    """layout "BSND": s1 an int (rows per sequence), seqused_q optional; "TND": s1 the list of rows per sequence.
    cmp: None / "dense" / "sparse"; sinks: "normal" / "off" / "hot"; index_rows(c, r, limit, K, rng) -> a row of K slots (default: as the
    indexer fills it: min(K, limit) distinct visible keys in random order, then -1); grid = (step of q, step of kv): values rounded to
    multiples of it (the stored reference cases: such files compress)."""
    rng = np.random.default_rng(seed)
    B = len(lens)
    c = dict(name=name, layout_q=layout, ori_block=ori_block, cmp_block=cmp_block, cmp_ratio=ratio if cmp else 1, ori_win_left=window[0],
             ori_win_right=window[1], softmax_scale=SCALE, seqused_kv=torch.tensor(lens, dtype=torch.int32), sparse_count=K, cmp_mode=cmp)
    if layout == "TND":
        c["cu_seqlens_q"] = torch.tensor(np.concatenate([[0], np.cumsum(s1)]), dtype=torch.int32)
        shape = (int(sum(s1)), HEADS, D)
    else:
        shape = (B, s1, HEADS, D)
        if seqused_q is not None:
            c["seqused_q"] = torch.tensor(seqused_q, dtype=torch.int32)
    c["q"] = torch.from_numpy(_grid(0.1 * rng.standard_normal(shape) + 0.05, grid[0]).astype(np.float32)).to(dtype)
    sk = 2.0 * rng.standard_normal(HEADS)
    if sinks == "off":
        sk[:] = -1.0e4
    elif sinks == "hot":
        sk[[3, 17, 40]] = 30.0
    c["sinks"] = torch.from_numpy(sk.astype(np.float32))
    rows = token_rows(c)
    # the keys somebody reads: windows first, then the compressed part (which needs a provisional cmp_base marker for token_list)
    used_ori = [set() for _ in range(B)]
    used_cmp = [set() for _ in range(B)]
    if cmp:
        c["cmp_base"] = True
    idx = torch.full((len(rows), max(K, 1)), -1, dtype=torch.int32) if cmp == "sparse" else None
    for r, (b, i, s1b) in enumerate(rows):
        lst = token_list(c, b, i, s1b)
        if lst is None:
            continue
        win, dense, limit = lst
        used_ori[b].update(win)
        if cmp == "dense":
            used_cmp[b].update(dense)
        elif cmp == "sparse":
            if index_rows is not None:
                row = index_rows(c, r, limit, K, rng)
            else:
                n = min(K, limit)
                row = np.concatenate([rng.permutation(limit)[:n], np.full(K - n, -1)])
            idx[r] = torch.tensor(np.asarray(row), dtype=torch.int32)
            used_cmp[b].update(int(j) for j in row if 0 <= j < limit)
    c["ori_base"], c["ori_block_table"] = _paged(rng, lens, ori_block, used_ori, dtype, grid[1])
    if cmp:
        c["cmp_base"], c["cmp_block_table"] = _paged(rng, [n // ratio for n in lens], cmp_block, used_cmp, dtype, grid[1])
    if idx is not None:
        c["cmp_sparse_indices"] = idx.reshape(*c["q"].shape[:-2], 1, K)
    return c


def ori_kv(c):
    return paged_view(c["ori_base"], c["ori_block"])


def cmp_kv(c):
    return None if c.get("cmp_base") is None else paged_view(c["cmp_base"], c["cmp_block"])


# ---- the case table of the GPU tests: six cases (a - f) in three row layouts each
def _layout(li, rot):
    """(layout, lens, s1, seqused_q): 0 = BSND decode over every length; 1 = BSND with S1 = 3 and seqused_q [3, 1, 0]; 2 = TND with
    cu_seqlens_q [0, 1, 4, 4, 6] (an empty sequence).  `rot` moves the lengths round so that the short layouts see different ones."""
    if li == 0:
        return "BSND", list(LENS), 1, None
    pick = [LENS[(rot + 3 * j) % len(LENS)] for j in range(4)]
    if li == 1:
        return "BSND", [pick[0], 129 if rot % 2 else 257, 640], 3, [3, 1, 0]
    return "TND", [1500 if rot % 2 else 255, 1, pick[2], pick[3]], [1, 3, 0, 2], None


SPECS = {      # name -> per layout: (cmp, ratio, window, sinks, K)
    "a": [(None, 1, (127, 0), "normal", 0)] * 3,
    "b": [(None, 1, (5, 2), "off", 0), (None, 1, (0, 0), "off", 0), (None, 1, (5, 2), "off", 0)],
    "c": [("dense", 128, (127, 0), "normal", 0)] * 3,
    "d": [("dense", 4, (5, 0), "normal", 0)] * 3,
    "e": [("sparse", 4, (127, 0), "normal", 512)] * 3,
    "f": [("sparse", 4, (5, 0), "hot", 64), ("sparse", 4, (5, 0), "hot", 1), ("sparse", 4, (5, 0), "hot", 64)],
}
VARIANTS = [(name, li) for name in SPECS for li in range(3)]
_cache = {}


def case(name, li, dtype, seed=None):
    """-> (case, restatement output); built and computed once, shared by the tests, never modified."""
    key = (name, li, dtype, seed)
    if key not in _cache:
        ci = "abcdef".index(name)
        cmp, ratio, window, sinks, K = SPECS[name][li]
        layout, lens, s1, sq = _layout(li, ci)
        if li == 0 and seed is not None:
            lens = [lens[(j + seed) % len(lens)] for j in range(len(lens))]
        ob, cb = BLOCK_PAIRS[(ci + li) % 3]
        c = make_case(f"{name}{li}", layout, lens, s1, ob, cb, cmp, ratio, window, sinks, K=K, dtype=dtype,
                      seed=1000 + 10 * ci + li + (0 if seed is None else 100 * seed), seqused_q=sq)
        _cache[key] = (c, attend_ref(c))
    return _cache[key]


def sharpness(c):
    """What the case's tokens exercise: {"cut by end", "cut by 0", "limit 0", "limit below K"}."""
    seen = set()
    idx = c.get("cmp_sparse_indices")
    for r, (b, i, s1b) in enumerate(token_rows(c)):
        lst = token_list(c, b, i, s1b)
        if lst is None:
            seen.add("zero row")
            continue
        L = int(c["seqused_kv"][b])
        p = L - s1b + i
        if p + c["ori_win_right"] >= L - 1:
            seen.add("cut by end")
        if p - c["ori_win_left"] <= 0:
            seen.add("cut by 0")
        if c.get("cmp_base") is not None:
            if lst[2] == 0:
                seen.add("limit 0")
            if idx is not None and lst[2] < c["sparse_count"]:
                seen.add("limit below K")
    return seen


# ---- stored outputs of the reference test's golden (tests/golden/gen_sparse_sharedkv_golden.py)
def golden_paths():
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_sharedkv_ref_*.npz")))


def load_golden(path):
    z = np.load(path)
    dtype = getattr(torch, str(z["dtype"]))
    bits = lambda a: torch.from_numpy(a.copy()).view(dtype)      # noqa: E731
    block = int(z["ori_block"])
    c = dict(name=os.path.basename(path), layout_q="BSND", q=bits(z["q_bits"]), ori_base=bits(z["ori_bits"]), ori_block=block, cmp_block=0,
             ori_block_table=torch.from_numpy(z["ori_block_table"].copy()), seqused_kv=torch.from_numpy(z["seqused_kv"].copy()),
             sinks=torch.full((HEADS,), -1.0e4), softmax_scale=float(z["softmax_scale"]), cmp_ratio=1, ori_win_left=int(z["ori_win_left"]),
             ori_win_right=int(z["ori_win_right"]), sparse_count=0, cmp_mode=None, golden_heads=z["heads"].copy(),
             golden=torch.from_numpy(z["golden"].copy()))
    return c
