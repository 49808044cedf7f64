"""Float64 restatement of the prefill block-score indexer (flash_prefill_bnsd_score, flash_prefill_bnsd_topk_from_score and the selection
of flash_prefill_bnsd_with_topk_idx) in plain loops over (request, token, head, block), the checks the CPU and GPU tests share, and the GPU
tests' case table.  Test infrastructure, like block_score_ref.py: the CPU test ties it to stored outputs of the reference kernel, the GPU
tests hold the HIP kernels to it.

Request r owns the tokens t in [cu[r], cu[r + 1]); L = seq_lens[r] clamped to [0, max_seqblock * bs]; page(r, j) =
req_to_token[req_pool_indices[r], min(j * bs, cols - 1)] // bs.  Key n of block j is visible to token t iff j * bs + n < L and
j * bs + n <= query_pos[t]; score[h, t, j] = max_n s ("max") or m + log2(sum_n exp2(s - m)) ("lse") over the visible keys,
s = (q[t, h] . k[page, n, h // G]) * sm_scale * log2(e), -inf when none is visible.  query_pos defaults to the token's TRUE position
seq_lens[r] - q_len[r] + i; the reference kernel compares with the PACKED index t (packed_positions).  Tokens at or behind cu[n] and a
negative position give all -inf rows.

TOL is block_score_ref.TOL: the same arithmetic (fp32 products of the same bf16 / fp16 inputs, head dims up to 256, max / exp2 / log2 in
float32).  test_block_score_prefill_cpu.py re-measures the fp32 error on every input below and requires it to be at most TOL / 2."""
import numpy as np
import torch

from block_score_ref import LOG2E, TOL, _np, check_row, select_ref  # noqa: F401

NEG = -np.inf


def true_positions(cu, seq_lens, total_q):
    """[total_q] int64: seq_lens[r] - q_len[r] + i for the tokens of request r; -1 for the tokens no request owns."""
    cu, sl = _np(cu, "i"), _np(seq_lens, "i")
    pos = np.full(total_q, -1, dtype=np.int64)
    for r in range(len(sl)):
        a, b = int(cu[r]), min(int(cu[r + 1]), total_q)
        for t in range(a, b):
            pos[t] = sl[r] - (cu[r + 1] - cu[r]) + (t - a)
    return pos


def packed_positions(total_q):
    """What the reference's score kernels compare the key position with: the packed token index."""
    return np.arange(total_q, dtype=np.int64)


def causal_lens(cu, seq_lens, total_q):
    """per_query_seq_lens of the true positions: position + 1 (0 for the tokens no request owns), int32."""
    return (true_positions(cu, seq_lens, total_q) + 1).astype(np.int32)


def prefill_scores_ref(q, k_cache, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size, max_seqlen, sm_scale, score_type="max",
                       query_pos=None, fp32=False):
    """-> score [Hidx, total_q, max_seqblock] float64 (-inf where nothing is visible).  fp32 = True: the same in float32 arithmetic (torch
    float32 matmul, float32 scaling and reductions) -- the comparison TOL is measured with."""
    cu, sl, rtt, rpi = _np(cu_seqlens, "i"), _np(seq_lens, "i"), _np(req_to_token, "i"), _np(req_pool_indices, "i")
    qd, kd = (q.detach().cpu().float(), k_cache.detach().cpu().float()) if fp32 else (_np(q, "f"), _np(k_cache, "f"))
    total_q, H, D = qd.shape
    bs, Hkv = kd.shape[1], kd.shape[2]
    assert bs == block_size and H % Hkv == 0
    G = H // Hkv
    msb = -(-int(max_seqlen) // bs)
    scale = np.float32(np.float32(sm_scale) * np.float32(LOG2E)) if fp32 else float(np.float32(sm_scale)) * LOG2E
    pos = true_positions(cu, sl, total_q) if query_pos is None else _np(query_pos, "i")
    out = np.full((H, total_q, msb), NEG, dtype=np.float64)
    for r in range(len(sl)):
        L = min(max(int(sl[r]), 0), msb * bs)
        for t in range(int(cu[r]), min(int(cu[r + 1]), total_q)):
            lim = min(L, int(pos[t]) + 1)
            for j in range(msb):
                n = min(bs, lim - j * bs)
                if n <= 0:
                    break
                page = int(rtt[int(rpi[r]), min(j * bs, rtt.shape[1] - 1)]) // bs
                for h in range(H):
                    if fp32:
                        s = (kd[page, :n, h // G] @ qd[t, h]) * torch.tensor(scale)
                        m = s.max()
                        v = float(m if score_type == "max" else m + torch.log2(torch.exp2(s - m).sum()))
                    else:
                        s = (kd[page, :n, h // G] @ qd[t, h]) * scale
                        m = s.max()
                        v = m if score_type == "max" else m + np.log2(np.exp2(s - m).sum())
                    out[h, t, j] = NEG if v != v else v
    return out


def topk_from_score_ref(score, per_query_seq_lens, topk, block_size):
    """flash_prefill_bnsd_topk_from_score, rank by rank: [H, total_q, nblk] -> [H, total_q, topk + 1] int64."""
    sc, lens = np.asarray(score, dtype=np.float64), _np(per_query_seq_lens, "i")
    H, T, nblk = sc.shape
    out = np.full((H, T, topk + 1), -1, dtype=np.int64)
    for h in range(H):
        for t in range(T):
            row = sc[h, t].copy()
            qpos = max(int(lens[t]) - 1, 0)
            for rank in range(topk):
                best = row.max()
                j = int(np.flatnonzero(row == best)[0])          # ties: the lowest block id
                if best > NEG and j * block_size <= qpos:
                    out[h, t, rank] = j
                row[j] = NEG
            local = min(qpos // block_size, nblk - 1)
            out[h, t, topk] = -1 if local in out[h, t, :topk].tolist() else local
    return out


def select_plain_ref(score, topk):
    """The non-fused selection: per row the min(topk, #finite) best blocks, descending, ties by ascending id, then -1."""
    sc = np.asarray(score, dtype=np.float64)
    H, T, _ = sc.shape
    out = np.full((H, T, topk), -1, dtype=np.int64)
    for h in range(H):
        for t in range(T):
            fin = [j for j in range(sc.shape[2]) if sc[h, t, j] > NEG]
            order = sorted(fin, key=lambda j: (-sc[h, t, j], j))[:topk]
            out[h, t, :len(order)] = order
    return out


def visible_blocks(score_row):
    """The visible blocks of a row are a prefix 0 .. nb - 1 (causal): -> nb."""
    fin = np.flatnonzero(np.asarray(score_row) > NEG)
    nb = len(fin)
    assert nb == 0 or fin[-1] == nb - 1, "visible blocks must be a prefix"
    return nb


def check_scores(got, want, tol=TOL):
    """Identical -inf pattern, finite scores within tol.  Returns the largest difference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any(), "NaN in the scores"
    fin = want > NEG
    assert np.array_equal(got > NEG, fin), "the -inf pattern differs"
    assert not np.isposinf(got).any()
    worst = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print("max |score - score_f64|", worst, "tol", tol)
    assert worst <= tol, worst
    return worst


def check_rows(got_idx, score, topk, fused_lens=None, block_size=None, max_ambiguous=0.02):
    """Every row of got_idx [H, total_q, topk (+ 1)] by block_score_ref.check_row against the float64 scores (positions at which every
    visible block is causally valid: the true ones); at most max_ambiguous of the rows may be ambiguous.  With fused_lens the appended slot
    must follow from the entries in front of it.  Returns the ambiguous count."""
    got_idx = _np(got_idx, "i")
    H, T = got_idx.shape[:2]
    amb = 0
    for h in range(H):
        for t in range(T):
            nb = visible_blocks(score[h, t])
            amb += bool(check_row(got_idx[h, t, :topk], score[h, t, :nb], True, topk, 0, 0))
            if fused_lens is not None:
                qpos = max(int(fused_lens[t]) - 1, 0)
                local = min(qpos // block_size, score.shape[2] - 1)
                assert got_idx[h, t, topk] == (-1 if local in got_idx[h, t, :topk].tolist() else local), (h, t, got_idx[h, t].tolist(), local)
    print("ambiguous rows", amb, "of", H * T)
    assert amb <= max_ambiguous * H * T, (amb, H * T)
    return amb


# ---- the GPU tests' case table (built on the CPU; test_block_score_prefill_cpu.py measures the fp32 error and the ambiguous rows on it) ----
# requests: (cached prefix, new tokens).  The score kernel's tile holds 64 // G tokens; a run of blocks holds 2048 keys.
#  name              Hidx Hkv  D   bs  requests                                        pad topk type  options
CASES = [
    # one request, no prefix: two full tiles and a part; blocks of 16
    ("mha_bs16",        2, 2, 64, 16, [(0, 150)], 0, 4, "max", dict()),
    # G = 4 (tiles of 16 tokens): a prefix inside a block, a prefix of whole blocks with one token, no token at all, no prefix with seq_len a
    # multiple of the block, seq_len a multiple of the block behind a prefix; padding tokens; int64 indices
    ("g4_bs64_lse",     4, 1, 128, 64, [(70, 37), (128, 1), (30, 0), (0, 64), (100, 92)], 3, 2, "lse", dict(idx_dtype=torch.int64)),
    # G = 20: tiles of 3 tokens in 60 of 64 rows, two 16-row blocks per token boundary; head dim 80; blocks of 128
    ("g20_d80_bs128",  20, 1, 80, 128, [(0, 50), (300, 33), (256, 17)], 5, 2, "max", dict(seed=1)),
    # two kv heads, head dim 256, a strided K view
    ("hkv2_g4_d256",    8, 2, 256, 32, [(33, 70), (0, 31)], 0, 3, "lse", dict(strided=True)),
    # a prefix longer than one run of blocks (2048 keys): two runs per tile, the second one diagonal
    ("mha_two_runs",    1, 1, 128, 32, [(2100, 130)], 0, 8, "max", dict()),
    # G = 80: one token per tile, two blocks of 64 heads
    ("g80_head_blocks", 80, 1, 64, 16, [(5, 9), (0, 3)], 2, 2, "lse", dict()),
]


def make_case(name, H, Hkv, D, bs, requests, pad, topk, score_type, opt, dtype):
    """CPU tensors of one case.  Every request owns its pages; one more page, which no request owns, and the rows behind each request's end
    inside its last block are NaN; req_to_token entries of blocks at or behind the end name the NaN page."""
    g = torch.Generator().manual_seed(opt.get("seed", 0) * 7919 + sum(map(ord, name)))
    idt = opt.get("idx_dtype", torch.int32)
    n = len(requests)
    lens = [a + b for a, b in requests]
    cu = np.concatenate([[0], np.cumsum([b for _, b in requests])])
    total_q = int(cu[-1]) + pad
    max_seqlen = max(lens)
    mb = -(-max_seqlen // bs)
    used = [-(-x // bs) for x in lens]
    num_pages = sum(used) + 1
    poison = num_pages - 1
    width = 2 * D if opt.get("strided") else D
    buf = torch.randn((num_pages, bs, Hkv, width), generator=g).to(dtype)
    k = buf[..., :D]                                           # strided: a view with rows 2 D apart
    q = torch.randn((total_q, H, D), generator=g).to(dtype)
    perm = torch.randperm(num_pages - 1, generator=g).tolist()
    rows, cols = n + 2, mb * bs + 5
    rtt = torch.full((rows, cols), poison * bs, dtype=torch.int64)
    pool = torch.tensor([rows - 1 - r for r in range(n)], dtype=torch.int64)
    for r in range(n):
        for j in range(used[r]):
            page = perm.pop()
            rtt[pool[r], j * bs:(j + 1) * bs] = page * bs + torch.arange(bs)
            if j == used[r] - 1 and lens[r] % bs:              # keys behind the end inside the last block
                k[page, lens[r] % bs:] = float("nan")
    k[poison] = float("nan")
    return dict(name=name, q=q, k=k, k_base=buf, cu_seqlens=torch.tensor(cu).to(idt), seq_lens=torch.tensor(lens).to(idt), req_to_token=rtt.to(idt),
                req_pool_indices=pool.to(idt), max_seqlen=max_seqlen, block_size=bs, topk=topk, score_type=score_type, sm_scale=float(D) ** -0.5,
                total_q=total_q, poison=poison)


def restate(c, query_pos=None, fp32=False, score_type=None):
    return prefill_scores_ref(c["q"], c["k"], c["cu_seqlens"], c["seq_lens"], c["req_to_token"], c["req_pool_indices"], c["block_size"],
                              c["max_seqlen"], c["sm_scale"], score_type or c["score_type"], query_pos=query_pos, fp32=fp32)


# ---- stored outputs of the reference kernels (tests/golden/block_score_prefill_ref_fp16_*.npz, gen_block_score_prefill_golden.py) ----------
def load_golden(path):
    """Cases a-c: inputs in make_case's layout plus fused, block_size_q, per_query_seq_lens (fused) and the reference's score and topk_idx.
    Case d: score, per_query_seq_lens, topk, block_size and the reference's topk_idx only."""
    z = np.load(path)
    c = dict(name=path, score=z["score"], want=z["topk_idx"].astype(np.int64), topk=int(z["topk"]), block_size=int(z["block_size"]),
             fused=bool(z["fused"]))
    if "per_query_seq_lens" in z.files:
        c["per_query_seq_lens"] = torch.from_numpy(z["per_query_seq_lens"])
    if "q" in z.files:
        for key in ("q", "k", "cu_seqlens", "seq_lens", "req_to_token", "req_pool_indices"):
            c[key] = torch.from_numpy(z[key])
        c.update(max_seqlen=int(z["max_seqlen"]), score_type=str(z["score_type"]), sm_scale=float(z["sm_scale"]), block_size_q=int(z["block_size_q"]),
                 total_q=c["q"].shape[0], packed_is_true=bool(z["packed_is_true"]))
    return c


def check_golden_rows(got, c):
    """got [H, total_q, topk (+ 1)] against the reference's stored rows: fused rows are equal; non-fused rows are equal on their first
    min(topk, #finite) entries (behind them the reference's torch.topk names arbitrary blocks) and ours hold -1 there."""
    got, want = _np(got, "i"), c["want"]
    assert got.shape == want.shape, (got.shape, want.shape)
    if c["fused"]:
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (bad[:5].tolist(), got[tuple(bad[0][:2])].tolist(), want[tuple(bad[0][:2])].tolist())
        return
    fin = (c["score"] > NEG).sum(axis=2)
    for h in range(got.shape[0]):
        for t in range(got.shape[1]):
            kk = min(c["topk"], int(fin[h, t]))
            assert got[h, t, :kk].tolist() == want[h, t, :kk].tolist(), (h, t, got[h, t].tolist(), want[h, t].tolist())
            assert all(x == -1 for x in got[h, t, kk:]), (h, t, got[h, t].tolist())


# ---- further inputs of the GPU tests, built on the CPU so that the CPU test can measure the fp32 error on them too -------------------------
def attention_case(dtype, seed=21):
    """End to end with the block-sparse prefill attention: one kv head, every row's visible blocks fit in topk, topk + 1 <= 64."""
    H, D, bs = 4, 128, 16
    c = make_case("attention", H, 1, D, bs, [(40, 70), (0, 33), (100, 1)], 0, 12, "max", dict(seed=seed), dtype)
    c["k"] = torch.nan_to_num(c["k"], nan=0.0)                 # the attention kernels are not part of the masked-data test
    g = torch.Generator().manual_seed(seed)
    c["v"] = torch.randn(c["k"].shape, generator=g).to(dtype)
    del c["k_base"]
    return c


def graph_cases():
    """Three problems of one shape on one K cache: cu_seqlens, seq_lens, the map and q differ.  max_seqlen (512) lies above every length."""
    H, Hkv, D, bs, total_q = 4, 2, 64, 32, 120
    out = []
    for i, reqs in enumerate(([(100, 50), (0, 70)], [(300, 100), (17, 20)], [(0, 1), (400, 112)])):
        c = make_case("graph", H, Hkv, D, bs, reqs, total_q - sum(b for _, b in reqs), 3, "lse", dict(seed=30 + i), torch.float16)
        out.append(c)
    pages = max(c["k"].shape[0] for c in out)
    first = out[0]
    g = torch.Generator().manual_seed(33)
    k = torch.randn((pages, bs, Hkv, D), generator=g).to(torch.float16)      # one cache for all three: every page is valid data
    cols = 512 + 5
    for c in out:
        rtt = torch.zeros((4, cols), dtype=torch.int32)
        rtt[:, :c["req_to_token"].shape[1]] = torch.where(c["req_to_token"] == c["poison"] * bs, 0, c["req_to_token"])
        c.update(k=k, req_to_token=rtt, max_seqlen=512)
        del c["k_base"]
    assert all(c["q"].shape == first["q"].shape for c in out)
    return out


def limits_case():
    """max_seqblock = 16384 with topk = 1024 on two tokens of a request of 1100 blocks (the select kernel's long-row form, the largest
    winner list)."""
    g = torch.Generator().manual_seed(9)
    H, D, bs, nb = 1, 64, 16, 1100
    rtt = torch.zeros((1, nb * bs), dtype=torch.int32)
    perm = torch.randperm(nb, generator=g)
    for j in range(nb):
        rtt[0, j * bs:(j + 1) * bs] = perm[j] * bs + torch.arange(bs, dtype=torch.int32)
    return dict(name="limits", q=torch.randn((2, H, D), generator=g).to(torch.float16), k=torch.randn((nb, bs, 1, D), generator=g).to(torch.float16),
                cu_seqlens=torch.tensor([0, 2], dtype=torch.int32), seq_lens=torch.tensor([nb * bs - 3], dtype=torch.int32), req_to_token=rtt,
                req_pool_indices=torch.tensor([0], dtype=torch.int32), max_seqlen=16384 * bs, block_size=bs, topk=1024, score_type="max",
                sm_scale=0.125, total_q=2)


def further_inputs():
    return [attention_case(torch.bfloat16), attention_case(torch.float16)] + graph_cases() + [limits_case()]
