"""Float64 restatement of the block-score indexer (flash_decode_bnsd_with_topk_idx, score-only form, and
append_local_block_to_topk_idx) in plain loops over (sequence, query head, block), the checks the CPU and GPU tests share, and the GPU
tests' case table.  Test infrastructure, like sparse_decode_ref.py: the CPU test ties it to stored outputs of the reference kernel, the GPU
tests hold the HIP kernels to it.

Per (b, h), kh = h // G: len = seq_lens[b] (packed: seq_lens[b * G + h % G]) clamped to [0, min(ceil(max_seqlen / bs), table columns) * bs],
nb = ceil(len / bs).  Block j < nb scores max_n s ("max") or m + log2(sum_n exp2(s - m)) ("lse") over s = (q . k[page, n, kh]) * sm_scale *
log2(e), keys n with j * bs + n < len -- the NATURAL score.  Then j < init_blocks -> 1e30, then j >= max(0, nb - local_blocks) -> 1e29.
The row is the min(topk, nb) blocks of highest score, descending, ties by ascending block id, then -1.  When the largest nb of the group
is <= topk, nothing is scored and the row is 0 .. nb - 1.

TOL.  A score computed in fp32 differs from its float64 value by rounding alone.  Measured on the CPU over every input of the tests (the
case table below in bf16 and fp16, and the stored reference cases), fp32 = torch float32 matmul of the same bf16 / fp16 inputs, scaling and
max / exp2 / log2 in float32: max |score_fp32 - score_f64| = MEASURED_FP32_ERROR below.  The figure depends on the order in which torch's
BLAS kernel sums the products, which differs between CPUs (1.23e-6 and 1.38e-6 were seen); the recorded one is the smaller, TOL does not
follow the machine, and test_block_score_cpu.py re-measures and requires the figure to lie between a quarter of the recorded one and TOL / 2.  TOL = 8 x that: the margin covers the MFMA's other summation order and the hardware exp2 / log2.  A GPU row
outside TOL is a finding to explain, not a reason to widen TOL."""
import numpy as np
import torch

MEASURED_FP32_ERROR = 1.24e-6      # 1.232e-6 on stored case d ("max"); 1.04e-6 on the case table
TOL = 8 * MEASURED_FP32_ERROR
LOG2E = 1.4426950408889634


def _np(t, kind):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu()
        return t.double().numpy() if kind == "f" else t.to(torch.int64).numpy()
    return np.asarray(t, dtype=np.float64 if kind == "f" else np.int64)


def _lens_and_blocks(seq_lens, B, G, bs, packed, max_seqlen, table_cols):
    cap = -(-int(max_seqlen) // bs)
    if table_cols is not None:
        cap = min(cap, table_cols)
    lens = np.clip(_np(seq_lens, "i"), 0, cap * bs).reshape(B, G if packed else 1)
    if not packed:
        lens = np.repeat(lens, G, axis=1)
    return lens, -(-lens // bs)                                # [B, G] each


def block_scores_ref(q, k_cache, seq_lens, block_size, max_seqlen, block_table=None, req_to_token=None, req_pool_indices=None, num_pages=None,
                     sanitize_page_ids=False, sm_scale=None, score_type="max", packed_seq_lens=False, fp32=False):
    """-> scores[b][h]: float64 array of the nb natural block scores of row (b, h).  fp32 = True: the same in float32 arithmetic (torch
    float32 matmul, float32 scaling and reductions) -- the comparison TOL is measured with."""
    bt, rtt, rpi = _np(block_table, "i"), _np(req_to_token, "i"), _np(req_pool_indices, "i")
    assert (bt is None) != (rtt is None) and (rtt is None) == (rpi is None)
    qd, kd = (q.detach().cpu().float(), k_cache.detach().cpu().float()) if fp32 else (_np(q, "f"), _np(k_cache, "f"))
    B, Hq, D = qd.shape
    bs, Hkv = kd.shape[1], kd.shape[2]
    assert bs == block_size and Hq % Hkv == 0
    G = Hq // Hkv
    scale = (D ** -0.5 if sm_scale is None else sm_scale)
    scale = np.float32(np.float32(scale) * np.float32(LOG2E)) if fp32 else float(np.float32(scale)) * LOG2E
    lens, nbs = _lens_and_blocks(seq_lens, B, G, bs, packed_seq_lens, max_seqlen, None if bt is None else bt.shape[1])
    out = []
    for b in range(B):
        rows = []
        for h in range(Hq):
            kh, n_len, nb = h // G, int(lens[b, h % G]), int(nbs[b, h % G])
            sc = np.empty(nb, dtype=np.float64)
            for j in range(nb):
                if bt is not None:
                    page = int(bt[b, j])
                else:
                    page = int(rtt[int(rpi[b]), min(j * bs, rtt.shape[1] - 1)]) // bs
                    if sanitize_page_ids:
                        page = min(max(page, 0), int(num_pages) - 1)
                n = min(bs, n_len - j * bs)
                if fp32:
                    s = (kd[page, :n, kh] @ qd[b, h]) * torch.tensor(scale)
                    m = s.max()
                    v = m if score_type == "max" else m + torch.log2(torch.exp2(s - m).sum())
                    sc[j] = float(v)
                else:
                    s = (kd[page, :n, kh] @ qd[b, h]) * scale
                    m = s.max()
                    sc[j] = m if score_type == "max" else m + np.log2(np.exp2(s - m).sum())
                if sc[j] != sc[j]:
                    sc[j] = -np.inf
            rows.append(sc)
        out.append(rows)
    return out


def forced_scores(natural, init_blocks, local_blocks):
    s = np.array(natural, dtype=np.float64)
    nb = len(s)
    s[:min(init_blocks, nb)] = 1e30
    if local_blocks > 0:
        s[max(0, nb - local_blocks):] = 1e29
    return s


def select_ref(natural, topk, init_blocks, local_blocks):
    """One row that was scored: the min(topk, nb) best blocks, descending score, ties by ascending id, then -1."""
    s = forced_scores(natural, init_blocks, local_blocks)
    order = sorted(range(len(s)), key=lambda j: (-s[j], j))[:topk]
    return order + [-1] * (topk - len(order))


def append_local_ref(topk_idx, seq_lens, block_size, num_blocks):
    """[H, B, topk] -> [H, B, topk + 1] (append_local_block_to_topk_idx); seq_lens [B]."""
    idx, lens = _np(topk_idx, "i"), _np(seq_lens, "i")
    H, B, topk = idx.shape
    out = np.full((H, B, topk + 1), -1, dtype=np.int64)
    for h in range(H):
        for b in range(B):
            qpos = max(int(lens[b]) - 1, 0)
            local = min(qpos // block_size, num_blocks - 1)
            for t in range(topk):
                v = int(idx[h, b, t])
                if 0 <= v < num_blocks and v * block_size <= qpos:
                    out[h, b, t] = v
            out[h, b, topk] = -1 if local in out[h, b, :topk].tolist() else local
    return out


def append_rows_ref(topk_idx, seq_lens, block_size, num_blocks, packed, G):
    """append_local_ref with the row's own length: seq_lens [B], or packed [B * G] (query head h reads entry b * G + h % G)."""
    idx, lens = _np(topk_idx, "i"), _np(seq_lens, "i")
    if not packed:
        return append_local_ref(idx, lens, block_size, num_blocks)
    return np.concatenate([append_local_ref(idx[h:h + 1], lens.reshape(-1, G)[:, h % G], block_size, num_blocks) for h in range(idx.shape[0])])


def block_topk_ref(q, k_cache, seq_lens, block_size, max_seqlen, topk, init_blocks, local_blocks, fused_append_local=False, max_num_blocks=None,
                   **kw):
    """-> (topk_idx [Hq, B, topk (+ 1)] int64, scores[b][h] float64 natural scores, scored[b][h] bool: False where the shortcut applied)."""
    scores = block_scores_ref(q, k_cache, seq_lens, block_size, max_seqlen, **kw)
    B, Hq = len(scores), len(scores[0])
    G = Hq // k_cache.shape[2]
    idx = np.full((Hq, B, topk), -1, dtype=np.int64)
    scored = [[True] * Hq for _ in range(B)]
    for b in range(B):
        for h in range(Hq):
            group = range(h // G * G, h // G * G + G)
            nb = len(scores[b][h])
            if max(len(scores[b][i]) for i in group) <= topk:
                idx[h, b, :nb] = np.arange(nb)
                scored[b][h] = False
            else:
                idx[h, b] = select_ref(scores[b][h], topk, init_blocks, local_blocks)
    if fused_append_local:
        idx = append_rows_ref(idx, seq_lens, block_size, max_num_blocks, kw.get("packed_seq_lens", False), G)
    return idx, scores, scored


def check_row(got, natural, scored, topk, init_blocks, local_blocks, tol=None):
    """The tolerant top-k check of one row `got` (topk entries) against the float64 natural scores.  Returns True when the row is
    AMBIGUOUS: the gap between the last natural block in and the best one out is within tol, so only the tolerant part was asserted."""
    tol = TOL if tol is None else tol
    got = [int(x) for x in got]
    nb = len(natural)
    k = min(topk, nb)
    assert all(0 <= x < nb for x in got[:k]) and len(set(got[:k])) == k, ("entries must be distinct blocks below nb", got, nb)
    assert all(x == -1 for x in got[k:]), ("-1 fills the tail and only the tail", got, nb)
    if not scored:
        assert got[:k] == list(range(k)), got
        return False
    want = select_ref(natural, topk, init_blocks, local_blocks)
    forced = set(range(min(init_blocks, nb))) | (set(range(max(0, nb - local_blocks), nb)) if local_blocks > 0 else set())
    assert [(t, x) for t, x in enumerate(got) if x in forced] == [(t, x) for t, x in enumerate(want) if x in forced], ("forced blocks", got, want)
    nat_got = [x for x in got[:k] if x not in forced]
    nat_want = [x for x in want[:k] if x not in forced]
    assert len(nat_got) == len(nat_want)
    kn = len(nat_got)
    others = sorted((natural[j] for j in range(nb) if j not in forced), reverse=True)
    if kn == 0:
        return False
    kth = others[kn - 1]
    assert all(natural[x] >= kth - tol for x in nat_got), ("a returned block lies below the k-th score by more than tol", got, want)
    assert all(natural[j] <= kth + tol for j in range(nb) if j not in forced and j not in nat_got), ("a better block was left out", got, want)
    ambiguous = kn < len(others) and kth - others[kn] <= tol
    if not ambiguous:
        assert set(nat_got) == set(nat_want), ("the boundary gap exceeds tol: the set must be the restatement's", got, want)
        sel = sorted(natural[x] for x in nat_want)
        if all(b - a > tol for a, b in zip(sel, sel[1:])):
            assert got == want, ("no ties: the order must be the restatement's", got, want)
    return ambiguous


def check_all(got_idx, scores, scored, topk, init_blocks, local_blocks, tol=None, max_ambiguous=0.02):
    """Every row of got_idx [Hq, B, >= topk]; at most max_ambiguous of the rows may be ambiguous.  Returns the ambiguous count."""
    got_idx = _np(got_idx, "i")
    Hq, B = got_idx.shape[:2]
    amb = sum(check_row(got_idx[h, b, :topk], scores[b][h], scored[b][h], topk, init_blocks, local_blocks, tol) for b in range(B) for h in range(Hq))
    print("ambiguous rows", amb, "of", Hq * B)
    assert amb <= max_ambiguous * Hq * B, (amb, Hq * B)
    return amb


# ---- the GPU tests' case table (built on the CPU; test_block_score_cpu.py measures the fp32 error and the ambiguous rows on it) ----------
L = 300 * 16
#  name             B Hq Hkv  D  bs topk  lens (per sequence; packed: per row)             init local type  options
CASES = [
    ("mha_bs16",       6, 2, 2, 64, 16, 3, [0, 1, 16, 17, 37, L], 1, 1, "max", dict()),
    ("g4_bs64_lse",    6, 8, 2, 128, 64, 8, [8 * 64, 8 * 64 + 1, 64, 65, 37, 3000], 2, 2, "lse", dict(seed=1)),      # seed 0: a 1.3e-6 near-tie in fp16
    ("g16_d80_bs128",  6, 16, 1, 80, 128, 1, [128, 129, 0, 1, 37, L], 0, 0, "max", dict(len_dtype=torch.int64, tab_dtype=torch.int64)),
    ("g32_direct",     4, 32, 1, 128, 16, 64, [64 * 16, 65 * 16, L, 37], 3, 70, "lse", dict(direct=True)),
    ("forced_gt_nb",   3, 8, 2, 64, 64, 3, [4 * 64 + 1, L, 64 * 4], 4, 4, "max", dict(strided=True)),
    ("packed_direct",  4, 8, 2, 128, 16, 8, [200, 216, 232, 248, 130, 131, 132, 133, 128, 128, 144, 129, 0, 150, 16, 160], 1, 1, "lse",
     dict(packed=True, direct=True, sanitize=True, tab_dtype=torch.int64, len_dtype=torch.int64)),
    ("g80_two_head_blocks", 2, 80, 1, 64, 32, 3, [37, 500], 0, 1, "lse", dict()),
    ("d256_bs32",      2, 4, 1, 256, 32, 2, [300, 37], 1, 0, "max", dict()),
    ("g4_max_nofor",   3, 16, 4, 128, 128, 8, [L, 128 * 9, 128 * 9 - 1], 0, 0, "max", dict(tab_dtype=torch.int64)),
    ("g32_d256",       2, 32, 1, 256, 64, 2, [300, 64 * 3 + 1], 0, 1, "lse", dict()),                     # 64 heads per workgroup at the widest rows
]


def make_case(name, B, Hq, Hkv, D, bs, topk, lens, init, local, score_type, opt, dtype):
    """CPU tensors of one case.  Every sequence owns its pages; one more page, which no sequence owns, and the rows behind each sequence's
    end inside its last block are NaN; table entries of blocks at or behind the end name the NaN page (direct map: its token slots)."""
    g = torch.Generator().manual_seed(opt.get("seed", 0) * 7919 + sum(map(ord, name)))
    G = Hq // Hkv
    packed = opt.get("packed", False)
    lens_t = torch.tensor(lens, dtype=opt.get("len_dtype", torch.int32))
    per_seq = lens_t.reshape(B, G).max(dim=1).values if packed else lens_t
    max_seqlen = int(per_seq.max())
    mb = max(1, -(-max_seqlen // bs))
    used = [-(-int(n) // bs) for n in per_seq]
    num_pages = sum(used) + 1
    poison = num_pages - 1
    width = 2 * D if opt.get("strided") else D
    buf = torch.randn((num_pages, bs, Hkv, width), generator=g).to(dtype)
    k = buf[..., :D]                                           # strided: a view with rows 2 D apart
    q = torch.randn((B, Hq, D), generator=g).to(dtype)
    perm = torch.randperm(num_pages - 1, generator=g).tolist()
    table = torch.full((B, mb), poison, dtype=torch.int64)
    for b in range(B):
        for j in range(used[b]):
            table[b, j] = perm.pop()
        if int(per_seq[b]) % bs:                               # keys behind the end inside the last block
            k[table[b, used[b] - 1], int(per_seq[b]) % bs:] = float("nan")
    k[poison] = float("nan")
    c = dict(name=name, q=q, k=k, k_base=buf, seq_lens=lens_t, max_seqlen=max_seqlen, block_size=bs, topk=topk, init_blocks=init, local_blocks=local,
             score_type=score_type, sm_scale=float(D) ** -0.5, packed=packed, max_num_blocks=mb)
    tab_dtype = opt.get("tab_dtype", torch.int32)
    if opt.get("direct"):
        rows, cols = B + 2, mb * bs + 5
        rtt = torch.full((rows, cols), poison * bs, dtype=torch.int64)
        pool = torch.tensor([rows - 1 - b for b in range(B)], dtype=torch.int64)
        for b in range(B):
            for j in range(used[b]):
                rtt[pool[b], j * bs:(j + 1) * bs] = table[b, j] * bs + torch.arange(bs)
        c.update(req_to_token=rtt.to(tab_dtype), req_pool_indices=pool.to(tab_dtype), num_pages=num_pages, sanitize=opt.get("sanitize", False))
    else:
        c["block_table"] = table.to(tab_dtype)
    return c


def ref_kwargs(c):
    """block_scores_ref / block_topk_ref keyword arguments of a case dict (make_case, or a stored reference case)."""
    kw = dict(sm_scale=c["sm_scale"], score_type=c["score_type"], packed_seq_lens=c.get("packed", False))
    if "req_to_token" in c:
        kw.update(req_to_token=c["req_to_token"], req_pool_indices=c["req_pool_indices"], num_pages=c["num_pages"],
                  sanitize_page_ids=c.get("sanitize", False))
    else:
        kw.update(block_table=c["block_table"])
    return kw


# ---- stored outputs of the reference kernel (tests/golden/block_score_ref_fp16_*.npz, written by gen_block_score_golden.py) --------------
def load_golden(path):
    """-> case dict in make_case's layout (CPU tensors) plus fused, knobs and want = the reference's topk_idx [Hq, B, topk (+ 1)]."""
    z = np.load(path)
    t = lambda key: torch.from_numpy(z[key])
    c = dict(name=path, q=t("q"), k=t("k"), seq_lens=t("seq_lens"), max_seqlen=int(z["max_seqlen"]), block_size=int(z["block_size"]),
             topk=int(z["topk"]), init_blocks=int(z["init_blocks"]), local_blocks=int(z["local_blocks"]), score_type=str(z["score_type"]),
             sm_scale=float(z["sm_scale"]), packed=bool(z["packed"]), max_num_blocks=int(z["max_num_blocks"]), fused=bool(z["fused"]),
             knobs={key[5:]: int(z[key]) for key in z.files if key.startswith("knob_")}, want=z["topk_idx"].astype(np.int64))
    if "req_to_token" in z.files:
        c.update(req_to_token=t("req_to_token"), req_pool_indices=t("req_pool_indices"), num_pages=int(z["num_pages"]), sanitize=bool(z["sanitize"]))
    else:
        c["block_table"] = t("block_table")
    return c


def check_golden(got, c):
    """got [Hq, B, topk (+ 1)] against the reference's stored rows: per row the first min(topk, nb) entries are equal as sets, and in order
    where no block is forced (among forced blocks the reference's order depends on its chunking); the reference's slots behind them are
    ignored (it repeats a candidate there) and ours must be -1; the appended slot is equal."""
    got, want = _np(got, "i"), c["want"]
    assert got.shape == want.shape, (got.shape, want.shape)
    Hq, B, topk = got.shape[0], got.shape[1], c["topk"]
    G = Hq // c["k"].shape[2]
    _, nbs = _lens_and_blocks(c["seq_lens"], B, G, c["block_size"], c["packed"], c["max_seqlen"],
                              c["block_table"].shape[1] if "block_table" in c else None)
    for h in range(Hq):
        for b in range(B):
            k = min(topk, int(nbs[b, h % G]))
            g, w = got[h, b].tolist(), want[h, b].tolist()
            assert set(g[:k]) == set(w[:k]) and len(set(g[:k])) == k, (h, b, g, w)
            if c["init_blocks"] == 0 and c["local_blocks"] == 0:
                assert g[:k] == w[:k], (h, b, g, w)
            assert all(x == -1 for x in g[k:topk]), (h, b, g)
            if c["fused"]:
                assert g[topk] == w[topk], (h, b, g, w)


# ---- further inputs of the GPU tests (pipeline, full form, graph replay, the declared limits): built on the CPU so that
# test_block_score_cpu.py can measure the fp32 error and the ambiguous rows on them too ---------------------------------------------------
def attention_case(B, Hq, Hkv, D, bs, lens, dtype, seed, sink=False, **more):
    g = torch.Generator().manual_seed(seed)
    mb = -(-max(lens) // bs)
    pages = B * mb
    c = dict(k=torch.randn((pages, bs, Hkv, D), generator=g).to(dtype), v=torch.randn((pages, bs, Hkv, D), generator=g).to(dtype),
             q=torch.randn((B, Hq, D), generator=g).to(dtype), block_table=torch.randperm(pages, generator=g).to(torch.int32).reshape(B, mb),
             seq_lens=torch.tensor(lens, dtype=torch.int32), max_seqlen=max(lens), block_size=bs, sm_scale=float(D) ** -0.5, max_num_blocks=mb,
             score_type="max", init_blocks=0, local_blocks=0)
    if sink:
        c["sink"] = (torch.randn((Hq, D), generator=g) * 1.5).to(dtype)
    c.update(more)
    return c


def full_form_case(dtype, score_type):
    return attention_case(3, 16, 2, 128, 64, [1500, 777, 64], dtype, seed=13, sink=True, topk=4, init_blocks=1, local_blocks=1, score_type=score_type)


def graph_cases():
    """Three problems of one shape on one K cache: lengths, block table and q differ.  max_seqlen (1024) lies above every length."""
    B, Hq, Hkv, D, bs = 3, 8, 2, 128, 16
    first = attention_case(B, Hq, Hkv, D, bs, [900, 300, 64], torch.float16, seed=5, topk=4, init_blocks=1, local_blocks=1, score_type="lse")
    first["max_seqlen"] = 1024
    g = torch.Generator().manual_seed(6)
    out = [first]
    for lens in ([100, 880, 1], [17, 0, 512]):
        out.append(dict(first, seq_lens=torch.tensor(lens, dtype=torch.int32), q=torch.randn((B, Hq, D), generator=g).to(torch.float16),
                        block_table=torch.randperm(first["k"].shape[0], generator=g).to(torch.int32).reshape(B, -1)))
    return out


def limits_case():
    """max_seqblock = 16384 (a row of scores fills 64 KB of LDS) and topk = 1024 (the largest sort) on a sequence of 1100 blocks."""
    g = torch.Generator().manual_seed(9)
    Hq, D, bs, nb = 2, 64, 16, 1100
    bt = torch.full((1, 16384), nb - 1, dtype=torch.int32)
    bt[0, :nb] = torch.randperm(nb, generator=g).to(torch.int32)
    return dict(q=torch.randn((1, Hq, D), generator=g).to(torch.float16), k=torch.randn((nb, bs, 1, D), generator=g).to(torch.float16),
                block_table=bt, seq_lens=torch.tensor([nb * bs - 3], dtype=torch.int32), max_seqlen=16384 * bs, block_size=bs, topk=1024,
                init_blocks=2, local_blocks=3, score_type="max", sm_scale=0.125, max_num_blocks=16384)


def further_inputs():
    return ([full_form_case(dt, st) for dt in (torch.bfloat16, torch.float16) for st in ("max", "lse")] + graph_cases() + [limits_case()])
