"""Float64 restatement of the lightning indexer (torch.ops.npu.lightning_indexer, csrc/kernels/lightning_indexer.hip), written from its
formula:  for a query row with index-query Q [64, 128], head weights w [64] and the keys K [S2, 128] of its sequence

    score[j] = sum_h w[h] * max(0, Q[h] . K[j])

and the row's result is the n = min(sparse_count, visible) visible keys of highest score, descending, ties by ascending key, then -1.
Visibility: sparse_mode 0: all act_s2 keys; sparse_mode 3: row r of the act_s1 query rows of a sequence sees keys j < act_s2 - (act_s1 - 1
- r), clamped at 0.  The stored reference results (tests/golden/lightning_indexer_ref_*.npz) differ from this in one documented way: the
reference test's golden fills min(sparse_count, act_s2) slots even when fewer keys are visible (masked keys in arbitrary order); here, as
in the HIP kernels, the row ends in -1.

bf16 / fp16 products are exact in fp32, so an fp32 evaluation differs from float64 by its summation order alone.  TOL[family] is a recorded
constant: 8 x the largest |score_fp32 - score_f64| measured once on the CPU over every test input of the family (the 8 x is the project's
margin for the MFMA's different order).  Families: "normal" (unit-normal Q, K, w: scores of some tens) and
"uniform" (the reference test's U(-10, 10) Q and K, U(-1, 1) w: scores about 1e3 times larger)."""
import functools
import os

import numpy as np
import torch

HEADS, DIM, MAX_SPARSE, MAX_KEYS = 64, 128, 2048, 262144
MEASURED_FP32_ERROR = {"normal": 9.0e-5, "uniform": 1.12e-3}         # test_lightning_indexer_cpu.py re-measures both
TOL = {f: 8 * v for f, v in MEASURED_FP32_ERROR.items()}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def visible_count(sparse_mode, act_s1, act_s2, r):
    if sparse_mode == 0:
        return act_s2
    return min(max(act_s2 - (act_s1 - 1 - r), 0), act_s2)


def scores_ref(q, w, k, fp32=False):
    """q [n, 64, 128], w [n, 64], k [s2, 128] (torch, bf16 / fp16) -> numpy [n, s2] float64 (fp32: every step in float32)."""
    dt = torch.float32 if fp32 else torch.float64
    n = q.shape[0]
    s = torch.clamp_min(k.to(dt) @ q.to(dt).reshape(n * HEADS, DIM).T, 0).reshape(-1, n, HEADS)      # [s2, n, 64]
    return (s * w.to(dt)[None]).sum(dim=2).T.double().numpy()


def select_ref(scores, visible, sparse_count):
    """Descending score, ties by ascending key, -1 behind the n winners."""
    s = np.asarray(scores[:visible], dtype=np.float64)
    order = np.lexsort((np.arange(len(s)), -s))
    out = np.full(sparse_count, -1, dtype=np.int32)
    n = min(sparse_count, visible)
    out[:n] = order[:n]
    return out


def sequences(c):
    """Per sequence b: (rows [list of global row ids], act_s1, act_s2).  BSND rows at or behind act_s1 belong to no sequence."""
    B = len(c["s2"])
    out, t = [], 0
    for b in range(B):
        s1 = c["s1"][b]
        if c["layout_query"] == "TND":
            rows = list(range(t, t + s1))
            t += s1
        else:
            rows = [b * c["S1"] + r for r in range(s1)]
        out.append((rows, s1, c["s2"][b]))
    return out


def keys_of(c, b, n):
    """The first n keys of sequence b, [n, 128]."""
    k = c["key"]
    if c["layout_key"] == "PA_BSND":
        bs = k.shape[1]
        nb = -(-n // bs)
        pages = c["block_table"][b, :nb].long()
        return k[pages].reshape(nb * bs, DIM)[:n]
    if c["layout_key"] == "BSND":
        return k[b, :n, 0]
    start = int(c["actual_seq_lengths_key"][b - 1]) if b else 0
    return k[start:start + n, 0]


def num_rows(c):
    return c["query"].shape[0] if c["layout_query"] == "TND" else c["query"].shape[0] * c["query"].shape[1]


def indexer_ref(c, fp32=False):
    """-> (idx [rows, sparse_count] int32, scores: per row a float64 array of its sequence's act_s2 scores (None: no sequence), visible
    per row)."""
    rows = num_rows(c)
    q = c["query"].reshape(rows, HEADS, DIM)
    w = c["weights"].reshape(rows, HEADS)
    K = c["sparse_count"]
    idx = np.full((rows, K), -1, dtype=np.int32)
    scores, visible = [None] * rows, [0] * rows
    for b, (rws, s1, s2) in enumerate(sequences(c)):
        if not rws:
            continue
        sc = scores_ref(q[rws], w[rws], keys_of(c, b, s2), fp32) if s2 > 0 else np.zeros((len(rws), 0))
        for r, row in enumerate(rws):
            visible[row] = visible_count(c["sparse_mode"], s1, s2, r)
            scores[row] = sc[r]
            idx[row] = select_ref(sc[r], visible[row], K)
    return idx, scores, visible


def free_keys(scores, visible, sparse_count, tol):
    """Keys other than the n-th best inside [s_n - tol, s_n + tol]: the ones the tolerant check cannot pin (0 when every visible key wins)."""
    n = min(sparse_count, visible)
    if n == 0 or n == visible:
        return 0
    s = np.asarray(scores[:visible])
    s_n = np.sort(s)[::-1][n - 1]
    return int((np.abs(s - s_n) <= tol).sum()) - 1


def check_row(idx, scores64, visible, sparse_count, tol):
    idx = np.asarray(idx).reshape(-1)
    assert idx.shape[0] == sparse_count
    n = min(sparse_count, visible)
    assert (idx[n:] == -1).all(), "a row ends in -1 behind its n entries"
    got = idx[:n].astype(np.int64)
    assert ((got >= 0) & (got < visible)).all(), "an entry outside [0, visible)"
    assert len(set(got.tolist())) == n, "duplicates"
    if n == 0:
        return
    s = np.asarray(scores64[:visible], dtype=np.float64)
    s_n = np.sort(s)[::-1][n - 1]
    member = np.zeros(visible, dtype=bool)
    member[got] = True
    assert member[s > s_n + tol].all(), "a key above the threshold is missing"
    assert not member[s < s_n - tol].any(), "a key below the threshold is present"
    sg = s[got]
    assert (sg[:-1] >= sg[1:] - 2 * tol).all(), "entries are not in descending order"
    same = sg[:-1] == sg[1:]
    assert (got[:-1][same] < got[1:][same]).all(), "equal scores must come in ascending key order"


def check_all(idx, scores, visible, sparse_count, tol):
    idx = np.asarray(idx).reshape(len(visible), sparse_count)
    for row, vis in enumerate(visible):
        check_row(idx[row], scores[row] if scores[row] is not None else np.zeros(0), vis, sparse_count, tol)


# ---------------------------------------------------------------------------------------------------------------- test inputs
def draw(shape, family, g, dtype, weights=False):
    if family == "normal":
        return torch.randn(shape, generator=g).to(dtype)
    lim = 1.0 if weights else 10.0
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * lim).to(dtype)


def make_case(name, lq, lk, s1, s2, block, count, mode, family="normal", S1=None, seed=0, extra_cols=1, poison=True, dtype=torch.bfloat16):
    """s1 / s2: the actual query rows / keys of every sequence.  Paged keys: pages in a permuted order out of one pool; with `poison`, NaN
    in every key row at or behind a sequence's length, a NaN page that every unused table entry names, and (BSND / TND keys) NaN rows behind
    the lengths."""
    g = torch.Generator().manual_seed(seed * 7919 + len(name))
    B = len(s2)
    c = dict(name=name, layout_query=lq, layout_key=lk, s1=list(s1), s2=list(s2), sparse_count=count, sparse_mode=mode, family=family)
    if lq == "TND":
        T = sum(s1)
        c["query"], c["weights"] = draw((T, HEADS, DIM), family, g, dtype), draw((T, HEADS), family, g, dtype, True)
        c["actual_seq_lengths_query"] = torch.tensor(np.cumsum(s1), dtype=torch.int32)
        c["S1"] = 1
    else:
        c["S1"] = S1 or max(s1)
        c["query"], c["weights"] = draw((B, c["S1"], HEADS, DIM), family, g, dtype), draw((B, c["S1"], HEADS), family, g, dtype, True)
        c["actual_seq_lengths_query"] = torch.tensor(s1, dtype=torch.int32) if list(s1) != [c["S1"]] * B else None
    bad = float("nan") if poison else 0.0
    if lk == "PA_BSND":
        nb = [-(-n // block) for n in s2]
        cols = max(nb) + extra_cols
        pool = sum(nb) + 2
        key = draw((pool, block, 1, DIM), family, g, dtype)
        perm = torch.randperm(pool - 1, generator=g).tolist()      # the last page belongs to nobody
        key[pool - 1] = bad
        table = torch.full((B, cols), pool - 1, dtype=torch.int32)
        for b in range(B):
            for j in range(nb[b]):
                table[b, j] = perm.pop()
            if s2[b] % block:
                key[table[b, nb[b] - 1], s2[b] % block:] = bad
        for page in perm:
            key[page] = bad
        c["key"], c["block_table"], c["capacity"] = key, table, cols * block
        c["actual_seq_lengths_key"] = torch.tensor(s2, dtype=torch.int32)
    elif lk == "BSND":
        cap = max(max(s2), 1) + 3
        key = draw((B, cap, 1, DIM), family, g, dtype)
        for b in range(B):
            key[b, s2[b]:] = bad
        c["key"], c["block_table"], c["capacity"] = key, None, cap
        c["actual_seq_lengths_key"] = torch.tensor(s2, dtype=torch.int32)
    else:
        total = sum(s2) + 3
        key = draw((total, 1, DIM), family, g, dtype)
        key[sum(s2):] = bad
        c["key"], c["block_table"], c["capacity"] = key, None, total
        c["actual_seq_lengths_key"] = torch.tensor(np.cumsum(s2), dtype=torch.int32)
    return c


# name, layout_query, layout_key, s1, s2, block, sparse_count, sparse_mode, options
CASES = [
    ("one_key", "TND", "PA_BSND", [1], [1], 16, 1, 3, {}),
    # visible below, at and above sparse_count around one 16-key unit; sparse_mode 0
    ("unit_edge", "TND", "PA_BSND", [1, 1, 1], [15, 16, 17], 16, 16, 0, {}),
    ("s2_255", "TND", "PA_BSND", [2], [255], 128, 3, 3, {}),
    # visible below, at and above sparse_count = 2048; blocks of 256
    ("count_edge", "BSND", "PA_BSND", [1, 1, 1], [2047, 2048, 2049], 256, 2048, 3, {}),
    # five rows of one sequence share every K load; a partly filled last page of 1024
    ("s2_4100", "TND", "PA_BSND", [5], [4100], 1024, 2048, 3, {}),
    # lengths far apart, an empty sequence, S1 per sequence 1 / 2 / 5, causal rows below / at / above sparse_count
    ("far_apart", "TND", "PA_BSND", [1, 2, 5], [4100, 0, 17], 16, 16, 3, {}),
    # causal rows whose visible count is <= 0, below and at sparse_count
    ("causal_short", "TND", "PA_BSND", [5], [3], 16, 3, 3, {}),
    # BSND with S1 = 4 and actual_seq_lengths_query shorter than S1
    ("bsnd_short_q", "BSND", "PA_BSND", [4, 2, 0], [300, 70, 50], 128, 16, 3, dict(S1=4)),
    ("key_bsnd", "BSND", "BSND", [2, 2], [100, 37], 0, 16, 0, {}),
    ("key_tnd", "TND", "TND", [2, 1], [70, 129], 0, 16, 3, {}),
    # a row that crosses every 16-bit and single-pass boundary of the select
    ("row_131072", "TND", "PA_BSND", [1], [131072], 128, 2048, 0, dict(extra_cols=0)),
    ("under_limit", "BSND", "PA_BSND", [1], [MAX_KEYS - 5], 1024, 16, 3, dict(extra_cols=0)),
    # the reference test's own distribution and shape
    ("reference_dist", "TND", "PA_BSND", [1, 2, 2], [8192, 8192, 8192], 256, 2048, 3, dict(family="uniform", extra_cols=0)),
]
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def case(name, dtype, poison=True):
    """A case of the table and its restatement, computed once per process and shared (treat both as read-only)."""
    spec = next(s for s in CASES if s[0] == name)
    c = make_case(*spec[:8], dtype=dtype, poison=poison, **spec[8])
    return c, indexer_ref(c)


def tie_case(kind, dtype):
    """Constructed ties (BSND keys, one sequence of two query rows, 601 keys, every key visible).  "dup": key 2i + 1 repeats key 2i, so every
    score comes twice and an odd sparse_count cuts a pair at the threshold; "zero": all weights 0, every score is 0; "neg": all weights
    negative, every score <= 0 (with the pairs of "dup")."""
    c = make_case("ties_" + kind, "BSND", "BSND", [2], [601], 0, 63, 0, seed=11, dtype=dtype)
    k = c["key"]
    k[0, 1:601:2] = k[0, 0:600:2]
    if kind == "zero":
        c["weights"] = torch.zeros_like(c["weights"])
    if kind == "neg":
        c["weights"] = -c["weights"].abs()
    return c


def graph_cases(dtype):
    """Two inputs of one shape (decode, three sequences) over one key cache: a captured graph replays the second in the buffers of the
    first.  The second has other queries and weights, the table rows in another order and other lengths (one of them 0)."""
    c1 = make_case("graph", "TND", "PA_BSND", [1, 1, 1], [700, 65, 130], 64, 16, 3, seed=21, extra_cols=3, dtype=dtype)
    g = torch.Generator().manual_seed(22)
    c2 = dict(c1, s2=[100, 663, 0], query=draw(c1["query"].shape, "normal", g, dtype), weights=draw(c1["weights"].shape, "normal", g, dtype),
              block_table=c1["block_table"][[2, 0, 1]].clone(), actual_seq_lengths_key=torch.tensor([100, 663, 0], dtype=torch.int32))
    return [c1, c2]


def slice_case(dtype):
    """13 rows in groups of four: with the workspace bound at two groups the op runs two slices."""
    return make_case("slices", "TND", "PA_BSND", [7, 6], [200, 90], 16, 16, 3, seed=31, dtype=dtype)


def further_inputs():
    out = []
    for dtype in DTYPES:
        out += [tie_case(k, dtype) for k in ("dup", "zero", "neg")] + graph_cases(dtype) + [slice_case(dtype)]
    return out


# ---------------------------------------------------------------------------------------------------------------- stored goldens
def _to_torch(a, dtype):
    return torch.from_numpy(a.copy()).view(dtype)


def load_golden(path):
    z = np.load(path)
    dtype = {"bfloat16": torch.bfloat16, "float16": torch.float16}[str(z["dtype"])]
    c = dict(name=os.path.basename(path), layout_query=str(z["layout_query"]), layout_key="PA_BSND", sparse_count=int(z["sparse_count"]),
             sparse_mode=int(z["sparse_mode"]), family=str(z["family"]), s1=z["s1"].tolist(), s2=z["s2"].tolist(), S1=int(z["S1"]),
             query=_to_torch(z["query_bits"], dtype), key=_to_torch(z["key_bits"], dtype), weights=_to_torch(z["weights_bits"], dtype),
             block_table=torch.from_numpy(z["block_table"].copy()), actual_seq_lengths_key=torch.from_numpy(z["actual_seq_lengths_key"].copy()),
             actual_seq_lengths_query=torch.from_numpy(z["actual_seq_lengths_query"].copy()) if "actual_seq_lengths_query" in z else None,
             golden=z["golden"])
    c["capacity"] = c["block_table"].shape[1] * c["key"].shape[1]
    return c


def golden_paths():
    import glob

    return sorted(glob.glob(os.path.join(GOLD, "lightning_indexer_ref_*.npz")))
