"""GPU parity: HIP paged MLA decode (through the C-ABI of include/mi_sgl_kernels.h) vs the CPU oracle, the committed
reference-kernel outputs, and (at BASELINE C4 size) an fp32 torch evaluation on the GPU.  Tolerance: 1e-3 absolute
(BASELINE.json north_star: "MLA decode matching reference within 1e-3") plus one output-dtype ulp."""
import ctypes
import glob
import os
from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from capi import load, ptr, stream_ptr
from oracle import kernels as OK

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load("libmi_sgl_kernels.so")
        _lib.mi_mla_decode_workspace.restype = c_size_t
        _lib.mi_mla_decode_workspace.argtypes = [c_int, c_int, c_int]
        _lib.mi_mla_decode_num_splits.argtypes = [c_int] * 4
        _lib.mi_mla_decode_plan_offset.restype = c_size_t
        _lib.mi_mla_decode_plan_offset.argtypes = [c_int, c_int]
        _lib.mi_mla_decode.argtypes = [c_void_p] * 6 + [c_int] * 6 + [c_int64] * 10 + [c_float, c_int, c_int, c_void_p, c_size_t, c_void_p]
    return _lib


def run_mla(q, kn, kr, lens, bt, sm_scale, num_splits=0, keep_ws=None):
    B, Hq, _ = q.shape
    Hkv = kn.shape[2]
    out = torch.empty((B, Hq, 512), dtype=q.dtype, device=q.device)
    max_len = int(lens.max().item()) if B else 0
    L = lib()
    if num_splits == 0:
        num_splits = L.mi_mla_decode_num_splits(B, Hq, Hkv, max_len)
    wsb = L.mi_mla_decode_workspace(B, Hq, num_splits)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=q.device)
    rc = L.mi_mla_decode(ptr(q), ptr(kn), ptr(kr), ptr(out), ptr(lens), ptr(bt), B, Hq, Hkv, kn.shape[1], bt.stride(0), max_len,
                         q.stride(0), q.stride(1), kn.stride(0), kn.stride(1), kn.stride(2), kr.stride(0), kr.stride(1),
                         kr.stride(2), out.stride(0), out.stride(1), sm_scale, 0 if q.dtype == torch.bfloat16 else 1,
                         num_splits, ptr(ws), wsb, stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if keep_ws is not None:
        keep_ws.append(ws)
    return out


@pytest.fixture(params=[4, 8, 9], ids=["wide4", "wide8", "wide8s"])
def wide_variant(request):
    """The three forms of the > 64-heads-per-group kernel (mla_decode_wide.hip, mla_decode_wide8.hip, mla_decode_wide8s.hip: 9 = eight
    waves, three KV slots, Q^T tail in LDS -- the default; page sizes that are not powers of two take the four-slot kernel there)."""
    assert lib().mi_mla_decode_select_wide(request.param) == 0
    yield request.param
    lib().mi_mla_decode_select_wide(0)


def tol(dtype):
    return dict(atol=1e-3, rtol=2 ** -7 if dtype == torch.bfloat16 else 2 ** -10)


PLANNED = -1      # MI_MLA_SPLITS_PLANNED: the device-built, length-aware work list (eight-wave wide kernel; others fall back to uniform splits)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "mla_ref_fp16_*.npz"))))
@pytest.mark.parametrize("splits", [1, 3, PLANNED])
def test_against_reference_kernel_outputs(path, splits, wide_variant):
    z = np.load(path)      # groups of <= 64 heads take the 64-head kernel whatever wide form is selected: checked under each selection
    t = lambda k: torch.from_numpy(z[k]).cuda()
    got = run_mla(t("q"), t("k_nope"), t("k_rope"), t("kv_seq_lens"), t("block_table"), float(z["sm_scale"]), splits)
    want = torch.from_numpy(z["out"]).cuda()
    assert torch.allclose(got.float(), want.float(), **tol(torch.float16)), (got.float() - want.float()).abs().max()


CASES = [  # B, Hq, Hkv, S, page, ragged
    (2, 16, 1, 200, 64, True), (4, 128, 1, 700, 64, True), (3, 32, 1, 129, 16, True), (2, 8, 1, 64, 128, False),
    (1, 64, 1, 1, 64, False), (2, 128, 1, 1314, 128, True), (2, 64, 8, 333, 32, True), (1, 256, 1, 150, 64, False),
    # wide (128-heads-per-workgroup) kernel edges: partially filled last wave, odd page size (integer-division path),
    # sequences shorter than one 32-key tile, two kv heads of 128, page_size 1
    (2, 96, 1, 200, 48, True), (3, 128, 1, 33, 64, True), (2, 128, 1, 1, 16, False), (1, 256, 2, 130, 64, True),
    (1, 128, 1, 70, 1, False), (1, 200, 1, 95, 32, False),
]


@pytest.mark.parametrize("B,Hq,Hkv,S,page,ragged", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("splits", [0, 1, 2, PLANNED])
def test_against_oracle(B, Hq, Hkv, S, page, ragged, dtype, splits, wide_variant):
    # groups of <= 64 heads take the 64-head kernel whatever wide form is selected: checked under each selection
    torch.manual_seed(2)
    maxp = (S + page - 1) // page
    nb = B * maxp + 3
    q = torch.randn((B, Hq, 576)).to(dtype)
    kn = torch.randn((nb, page, Hkv, 512)).to(dtype)
    kr = torch.randn((nb, page, Hkv, 64)).to(dtype)
    bt = torch.randperm(nb)[:B * maxp].to(torch.int32).reshape(B, maxp)
    lens = torch.tensor([max(1, S - 37 * i) if ragged else S for i in range(B)], dtype=torch.int32)
    sm = 1.0 / 576 ** 0.5
    want = OK.decode_mla(q, kn, kr, lens, bt, sm)
    got = run_mla(q.cuda(), kn.cuda(), kr.cuda(), lens.cuda(), bt.cuda(), sm, splits).cpu()
    if dtype == torch.float16:
        assert torch.allclose(got.float(), want.float(), **tol(dtype)), (got.float() - want.float()).abs().max()
        return
    # bf16: P is rounded to 8 bits before P.V (reference decode_attention.py:152); kernel and oracle round P against different
    # (equally valid) softmax references, so neither is the other's bit pattern.  Both are measured against the exact fp64 result,
    # in the form the full-C4 test uses: every element within 8e-3 of its head's output scale (half a bf16 ulp of the row scale is
    # 2^-9 = 2e-3, the P rounding comes on top), cosine distance < 1e-5 -- and the kernel must be as accurate as the oracle.
    exact = torch.zeros_like(want, dtype=torch.float64)
    group = Hq // Hkv
    for b in range(B):
        L = int(lens[b])
        idx = bt[b, :(L + page - 1) // page].long()
        for kvh in range(Hkv):
            K = torch.cat([kn[idx, :, kvh].reshape(-1, 512), kr[idx, :, kvh].reshape(-1, 64)], 1)[:L].double()
            hs = slice(kvh * group, (kvh + 1) * group)
            exact[b, hs] = torch.softmax((q[b, hs].double() @ K.T) * sm, -1) @ K[:, :512]
    scale = exact.abs().amax(dim=-1, keepdim=True).clamp_min(1e-6)                   # per (sequence, head)
    rel_k = ((got.double() - exact).abs() / scale).max().item()
    rel_o = ((want.double() - exact).abs() / scale).max().item()
    g64 = got.double()
    cos = 1.0 - (2 * (g64 * exact).sum() / (g64.pow(2).sum() + exact.pow(2).sum())).item()
    assert rel_k < 8e-3, (rel_k, rel_o)
    assert cos < 1e-5, cos
    assert rel_k <= 1.5 * rel_o + 1e-3, (rel_k, rel_o)


def test_full_size_c4_vs_fp32(wide_variant):
    """BASELINE C4: B=128, 128 q-heads, one latent KV head, D=576, page 64, seqlen 4096 (+ a ragged copy)."""
    torch.manual_seed(0)
    B, Hq, S, page = 128, 128, 4096, 64
    maxp = S // page
    nb = B * maxp
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(torch.bfloat16)
    kn = torch.randn((nb, page, 1, 512), generator=g, device="cuda").to(torch.bfloat16)
    kr = torch.randn((nb, page, 1, 64), generator=g, device="cuda").to(torch.bfloat16)
    bt = torch.randperm(nb, device="cuda").to(torch.int32).reshape(B, maxp)
    for ragged in (False, True):
        lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
        if ragged:
            lens = torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32)
        got = run_mla(q, kn, kr, lens, bt, 576 ** -0.5)
        # the WHOLE batch against an fp32 evaluation on the GPU (one-shot softmax): BASELINE's bar is 1e-3, and since the outputs
        # at this size are ~0.016 in magnitude an absolute 1e-3 would be a 6 % check -- so it is asserted per element RELATIVE to
        # the output scale of its row, plus the reference tests' cosine metric (tests/python/deepep/utils.py:191-195 form)
        worst_rel, worst_cos = 0.0, 0.0
        for b in range(B):
            L = int(lens[b])
            idx = bt[b, :(L + page - 1) // page].long()
            K = torch.cat([kn[idx].reshape(-1, 512), kr[idx].reshape(-1, 64)], dim=1)[:L].float()
            s = (q[b].float() @ K.T) * 576 ** -0.5
            ref = torch.softmax(s, dim=-1) @ K[:, :512]
            gb = got[b].float()
            scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-6)              # per head
            rel = ((gb - ref).abs() / scale).max().item()
            cos = 1.0 - (2 * (gb.double() * ref.double()).sum() / (gb.double().pow(2).sum() + ref.double().pow(2).sum())).item()
            worst_rel, worst_cos = max(worst_rel, rel), max(worst_cos, cos)
        # bf16 outputs: half an ulp of the row scale is 2^-9 = 2e-3 at most; P is rounded to bf16 before P.V on top of that
        assert worst_rel < 8e-3, worst_rel
        assert worst_cos < 1e-5, worst_cos


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("splits", [1, 2, PLANNED])
def test_growing_scores_take_the_rescaling_path(dtype, splits, wide_variant):
    """128-head groups run a kernel that fixes the softmax reference at the first tile; sequences whose later scores
    outgrow it (here by ~90 nats) are flagged and recomputed by the rescaling kernel.  Mixed batch: one such sequence,
    one ordinary."""
    torch.manual_seed(4)
    B, Hq, S, page = 2, 128, 512, 64
    maxp = S // page
    nb = B * maxp
    q = torch.randn((B, Hq, 576)).to(dtype)
    kn = torch.randn((nb, page, 1, 512)).to(dtype)
    kr = torch.randn((nb, page, 1, 64)).to(dtype)
    bt = torch.arange(nb, dtype=torch.int32).reshape(B, maxp)
    # sequence 0: keys 300.. point along q[0, 5] (score ~ |q|^2 * sm * 4), earlier keys are ordinary
    kn[bt[0, 5:].long()] = (4.0 * q[0, 5, :512]).to(dtype)[None, None, None, :] + 0.05 * kn[bt[0, 5:].long()]
    lens = torch.tensor([S, S - 100], dtype=torch.int32)
    sm = 1.0 / 576 ** 0.5
    want = OK.decode_mla(q, kn, kr, lens, bt, sm)
    got = run_mla(q.cuda(), kn.cuda(), kr.cuda(), lens.cuda(), bt.cuda(), sm, splits).cpu()
    assert torch.isfinite(got.float()).all()
    assert torch.allclose(got.float(), want.float(), rtol=2e-2, atol=2e-2), (got.float() - want.float()).abs().max()


def plan_reference(lens, kv_heads, workers, tile=32, min_tiles=8, max_splits=64, sort_max=2048, align=2):
    """The work list of the planned form restated on the host (sgl-kernel-npu_amd/csrc/kernels/decode_plan.h, decode_plan_kernel): piece size
    x = the smallest for which all pieces fit one round of workgroups; the pieces of a (sequence, kv head) pair are consecutive items, pairs
    in order of descending length (ties: lower index first).  -> (n_items, x, first[s], n[s], items {index: (pair, first tile, end tile, k, n)})."""
    seqs = len(lens) * kv_heads
    tiles = [(max(int(lens[s // kv_heads]), 0) + tile - 1) // tile for s in range(seqs)]
    pieces = lambda t, x: max(1, min((t + x - 1) // x, max_splits, t // min_tiles))
    x = max(max(tiles), 1)
    if seqs <= sort_max and seqs < workers:
        x = next(x for x in range(max(1, (sum(tiles) + workers - 1) // workers), max(max(tiles), 1) + 1)
                 if sum(pieces(t, x) for t in tiles) <= workers)
        n = [pieces(t, x) for t in tiles]
    else:
        n = [1] * seqs
    order = sorted(range(seqs), key=lambda s: (-tiles[s], s)) if seqs <= sort_max else list(range(seqs))
    first, at = [0] * seqs, 0
    for s in order:
        first[s] = at
        at += n[s]
    items = {}
    for s in range(seqs):
        per = ((tiles[s] + n[s] - 1) // n[s] + align - 1) // align * align      # pieces start on even tiles: the list also serves 64-key tiles
        for k in range(n[s]):
            items[first[s] + k] = (s, min(tiles[s], k * per), min(tiles[s], (k + 1) * per), k, n[s])
    return at, x, first, n, items


@pytest.mark.parametrize("B,Hq,Hkv,S,page,kind", [(128, 128, 1, 4096, 64, "uniform"), (128, 128, 1, 4096, 64, "ragged"), (37, 128, 1, 3000, 16, "ragged"),
                                                   (5, 256, 2, 9000, 64, "ragged"), (300, 128, 1, 700, 64, "ragged"), (16, 128, 1, 20000, 128, "one_long"),
                                                   # groups of <= 64 heads (TP shards): the 64-head kernel reads the same list, any page size
                                                   (128, 16, 1, 4096, 64, "ragged"), (9, 64, 4, 3000, 16, "ragged"), (40, 32, 1, 5000, 48, "ragged"),
                                                   (16, 8, 1, 20000, 128, "one_long"), (3, 128, 8, 4500, 64, "ragged"),
                                                   # a handful of very long sequences: up to 64 pieces each, so that they still fill the chip
                                                   (4, 128, 1, 33000, 64, "uniform"), (2, 16, 1, 50000, 64, "ragged"),
                                                   # more sequences than the list sorts (2048): batch order, one piece each
                                                   (2100, 16, 1, 130, 16, "ragged"), (1100, 128, 2, 100, 32, "ragged")])
def test_planned_work_list_matches_its_restatement_and_outputs_match_uniform_splits(B, Hq, Hkv, S, page, kind):
    """The device-built work list (length-aware split counts, the pieces of a sequence consecutive, sequences longest first) against its host
    restatement, word for word; structural properties (every tile of every sequence covered exactly once; padding only); and the
    outputs of the planned launch against the same kernel with ONE piece per sequence (no merge at all): equal within the fp32
    summation-order tolerance of a flash-decoding merge."""
    L = lib()
    assert L.mi_mla_decode_select_wide(8) == 0
    try:
        g = torch.Generator(device="cuda").manual_seed(B * 7 + S)
        maxp = (S + page - 1) // page
        nb = B * maxp
        dt = torch.bfloat16
        q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(dt)
        kn = (torch.randn((nb, page, Hkv, 512), generator=g, device="cuda") * 0.5).to(dt)
        kr = (torch.randn((nb, page, Hkv, 64), generator=g, device="cuda") * 0.5).to(dt)
        bt = torch.randperm(nb, generator=g, device="cuda").to(torch.int32).reshape(B, maxp)
        if kind == "uniform":
            lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
        elif kind == "ragged":
            lens = torch.randint(0, S + 1, (B,), generator=g, device="cuda").to(torch.int32)      # zero-length sequences included
        else:
            lens = torch.randint(1, 300, (B,), generator=g, device="cuda").to(torch.int32)
            lens[3] = S
        keep = []
        got = run_mla(q, kn, kr, lens, bt, 576 ** -0.5, PLANNED, keep_ws=keep)
        one = run_mla(q, kn, kr, lens, bt, 576 ** -0.5, 1)
        nz = lens.cpu() > 0
        assert torch.allclose(got.float()[nz], one.float()[nz], rtol=2 ** -7, atol=2e-3), (got.float()[nz] - one.float()[nz]).abs().max()
        # the work list itself
        workers = L.mi_mla_decode_plan_workers()
        off = L.mi_mla_decode_plan_offset(B, Hq)
        seqs = B * Hkv
        words = keep[0][off:].view(torch.int32).cpu().numpy()
        n_items, x, first, n, items = plan_reference(lens.cpu().tolist(), Hkv, workers)
        items_max = (seqs + workers + 7) // 8 * 8
        assert words[0] == n_items == sum(n) and n_items <= items_max and words[1] == x
        if seqs < workers:
            assert n_items <= workers, "every piece runs in the first round of workgroups"
            # ... on every XCD too: workgroup i runs on XCD i mod 8, and the items are the indices 0 .. n_items - 1
            assert max(sum(1 for i in items if i % 8 == xcd) for xcd in range(8)) <= (workers + 7) // 8
        info = words[16:16 + 2 * seqs].reshape(seqs, 2)
        assert list(info[:, 0]) == first and list(info[:, 1]) == n
        it = words[16 + 2 * seqs:16 + 2 * seqs + 4 * items_max].reshape(items_max, 4)
        covered = {}
        for i in range(items_max):
            if i in items:
                s, t0, t1, k, ns = items[i]
                assert tuple(it[i]) == (s, t0, t1, k | (ns << 8)), (i, tuple(it[i]), items[i])
                covered.setdefault(s, []).append((t0, t1, i, k))
            else:
                assert it[i][0] == -1, (i, tuple(it[i]))
        tiles_of = lambda s: (max(int(lens[s // Hkv]), 0) + 31) // 32
        for s in range(seqs):
            pieces = sorted(covered[s], key=lambda p_: p_[3])
            tiles = tiles_of(s)
            assert pieces[0][0] == 0 and pieces[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
            assert all(a[0] % 2 == 0 or a[0] == a[1] == tiles for a in pieces), "pieces start on 64-key boundaries (empty trailing ones: at the end)"
            assert [p_[2] for p_ in pieces] == list(range(first[s], first[s] + n[s])), "the pieces of a sequence are consecutive items"
        if seqs <= 2048:
            by_first = sorted(range(seqs), key=lambda s: first[s])
            assert all(tiles_of(a) >= tiles_of(b) for a, b in zip(by_first, by_first[1:])), "longest sequence first"
        if B * Hkv <= 4 and kind == "uniform":
            assert sum(n) > workers // 2 and max(n) > 16, "few long sequences are cut into enough pieces to fill the chip"
        if kind == "one_long":
            assert n[3 * Hkv] > 4          # the one long sequence is cut into many pieces, the short ones stay whole
    finally:
        L.mi_mla_decode_select_wide(0)


def test_plan_once_run_many_equals_the_per_call_plan():
    """decode_mla_plan + decode_mla(..., plan=...) (the work list built once and shared by calls on the same kv_seq_lens) against the
    default call that builds its own list: the same bits, on ragged batches of 128-head and of 16-head (TP shard) calls -- ONE list format
    serves both kernels; a shape the planned form does not serve (256 heads on one kv head) falls back to the plain call."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgl-kernel-npu_amd", "python"))
    from sgl_kernel_npu.attention.decode_attention import decode_mla, decode_mla_plan
    g = torch.Generator(device="cuda").manual_seed(21)
    for B, Hq, S, page in ((48, 128, 3000, 64), (48, 16, 3000, 64), (6, 256, 500, 64)):
        maxp = (S + page - 1) // page
        nb = B * maxp
        q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(torch.bfloat16)
        kn = (torch.randn((nb, page, 1, 512), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
        kr = (torch.randn((nb, page, 1, 64), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
        bt = torch.randperm(nb, generator=g, device="cuda").to(torch.int32).reshape(B, maxp)
        lens = torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32)
        want = torch.empty((B, Hq, 512), dtype=torch.bfloat16, device="cuda")
        decode_mla(q, kn, kr, want, lens, 576 ** -0.5, page, bt)
        plan = decode_mla_plan(lens, 1)
        for _ in range(3):
            got = torch.empty_like(want)
            decode_mla(q, kn, kr, got, lens, 576 ** -0.5, page, bt, plan=plan)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
        # the default call shares the list between calls on the SAME kv_seq_lens tensor (the layers of a step); an in-place write to the
        # tensor (a new step) rebuilds it: always the bits of a call that builds its own list (num_splits = -1)
        for step in range(3):
            if step:
                lens.copy_(torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32))
            own = torch.empty_like(want)
            torch.ops.npu.decode_mla(q, kn, kr, own, lens, 576 ** -0.5, page, bt, -1)
            for _ in range(3):
                got = torch.empty_like(want)
                decode_mla(q, kn, kr, got, lens, 576 ** -0.5, page, bt)
                torch.cuda.synchronize()
                assert torch.equal(got, own), step
        # a STALE list (built from other lengths: the previous step's, or another batch that lived in the same buffer) costs balance, never
        # correctness: the pieces are clamped to the tiles every sequence has now and the last piece runs to their end
        for other in (torch.clamp(lens - 37, min=0), torch.clamp(lens + 150, max=S), torch.randint(0, S + 1, (B,), generator=g, device="cuda").to(torch.int32)):
            want2 = torch.empty_like(want)
            decode_mla(q, kn, kr, want2, other, 576 ** -0.5, page, bt)
            got2 = torch.empty_like(want)
            decode_mla(q, kn, kr, got2, other, 576 ** -0.5, page, bt, plan=plan)
            torch.cuda.synchronize()
            nz = other.cpu() > 0
            assert torch.allclose(got2.float()[nz], want2.float()[nz], rtol=2 ** -7, atol=2e-3), (got2.float()[nz] - want2.float()[nz]).abs().max()


def test_decode_mla_in_a_captured_graph_shares_the_list_inside_the_capture_only():
    """Three decode_mla calls (layers of a step) captured in one HIP graph: the first builds the work list inside the graph, the others reuse
    it; every replay follows the CURRENT contents of kv_seq_lens (written in place between replays), and an eager call between capture
    and first replay does not pick up the captured (still empty) list."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgl-kernel-npu_amd", "python"))
    from sgl_kernel_npu.attention.decode_attention import decode_mla
    g = torch.Generator(device="cuda").manual_seed(5)
    B, Hq, S, page = 24, 128, 2500, 64
    maxp = (S + page - 1) // page
    nb = B * maxp
    q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(torch.bfloat16)
    kn = (torch.randn((nb, page, 1, 512), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    kr = (torch.randn((nb, page, 1, 64), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    bt = torch.randperm(nb, generator=g, device="cuda").to(torch.int32).reshape(B, maxp)
    lens = torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32)
    outs = [torch.empty((B, Hq, 512), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for o in outs:                                   # warm-up outside the capture (allocations, kernel attributes)
            decode_mla(q, kn, kr, o, lens, 576 ** -0.5, page, bt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for o in outs:
            decode_mla(q, kn, kr, o, lens, 576 ** -0.5, page, bt)
    # eager call before the first replay: its own list, not the captured one
    eager = torch.empty_like(outs[0])
    decode_mla(q, kn, kr, eager, lens, 576 ** -0.5, page, bt)
    own = torch.empty_like(outs[0])
    torch.ops.npu.decode_mla(q, kn, kr, own, lens, 576 ** -0.5, page, bt, -1)
    torch.cuda.synchronize()
    assert torch.equal(eager, own)
    for step in range(3):
        if step:
            lens.copy_(torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32))
        for o in outs:
            o.fill_(7.0)
        graph.replay()
        torch.ops.npu.decode_mla(q, kn, kr, own, lens, 576 ** -0.5, page, bt, -1)
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, own), step


def test_padded_kv_seq_lens_and_foreign_plans():
    """The batch is q's (reference decode_attention.py:178): a kv_seq_lens longer than q.size(0) (padded / graph-static buffer) is cut to the
    batch before the work list is built -- list builder and consumers must agree on the (sequence, kv head) pair count the item offsets are
    derived from --, a list built for ANOTHER batch size is refused instead of read with the wrong offsets, and the plan cache neither pins the
    caller's tensor nor survives clear_mla_plan_cache()."""
    import gc
    import sys
    import weakref
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgl-kernel-npu_amd", "python"))
    from sgl_kernel_npu.attention.decode_attention import decode_mla, decode_mla_plan
    g = torch.Generator(device="cuda").manual_seed(77)
    B, Hq, S, page, PAD = 20, 128, 1500, 64, 64
    maxp = (S + page - 1) // page
    nb = B * maxp
    q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(torch.bfloat16)
    kn = (torch.randn((nb, page, 1, 512), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    kr = (torch.randn((nb, page, 1, 64), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    bt = torch.randperm(nb, generator=g, device="cuda").to(torch.int32).reshape(B, maxp)
    padded = torch.full((PAD,), 10 ** 6, dtype=torch.int32, device="cuda")        # garbage behind the batch must never be read as lengths
    padded[:B] = torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32)
    want = torch.empty((B, Hq, 512), dtype=torch.bfloat16, device="cuda")
    decode_mla(q, kn, kr, want, padded[:B].clone(), 576 ** -0.5, page, bt)
    for _ in range(3):                                    # the cut view shares storage + version counter: calls 2, 3 reuse the list
        got = torch.empty_like(want)
        decode_mla(q, kn, kr, got, padded, 576 ** -0.5, page, bt)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    big = decode_mla_plan(padded, 1)                      # a list for 64 pairs is not a list for 20
    with pytest.raises(RuntimeError, match="plan does not belong"):
        torch.ops.npu.decode_mla_planned(q, kn, kr, torch.empty_like(want), padded[:B].contiguous(), 576 ** -0.5, page, bt, big)
    # the cache holds a weak reference: dropping the lengths tensor frees its storage
    lens = padded[:B].clone()
    decode_mla(q, kn, kr, torch.empty_like(want), lens, 576 ** -0.5, page, bt)
    torch.cuda.synchronize()
    probe = weakref.ref(lens.untyped_storage())
    del lens
    gc.collect()
    assert probe() is None, "the plan cache kept the caller's kv_seq_lens alive"
    torch.ops.npu.clear_mla_plan_cache()
    got = torch.empty_like(want)
    decode_mla(q, kn, kr, got, padded, 576 ** -0.5, page, bt)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert lib().mi_mla_decode_uniform_splits(B, Hq, 1, S) >= 1


def test_graph_replay_with_lengths_crossing_piece_boundaries():
    """A graph that captured decode_mla WITH a list built eagerly replays that list forever: it is as stale as the lengths written between
    replays make it.  Sequences that grow or shrink ACROSS the piece boundaries of the captured list (half, double, one key, a ramp, just
    over / under a boundary) still produce the result of a call that builds its own list (fp32 summation order differs with the piece
    cut: tolerance of the stale-list test above)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgl-kernel-npu_amd", "python"))
    from sgl_kernel_npu.attention.decode_attention import decode_mla, decode_mla_plan
    g = torch.Generator(device="cuda").manual_seed(9)
    B, Hq, S, page = 16, 128, 4096, 64
    maxp = S // page
    nb = B * maxp
    q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(torch.bfloat16)
    kn = (torch.randn((nb, page, 1, 512), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    kr = (torch.randn((nb, page, 1, 64), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    bt = torch.randperm(nb, generator=g, device="cuda").to(torch.int32).reshape(B, maxp)
    lens = torch.full((B,), 2048, dtype=torch.int32, device="cuda")
    out = torch.empty((B, Hq, 512), dtype=torch.bfloat16, device="cuda")
    plan = decode_mla_plan(lens, 1)                       # 16 sequences x 64 tiles on 256 workers: 16 pieces of 4 tiles each
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        decode_mla(q, kn, kr, out, lens, 576 ** -0.5, page, bt, plan=plan)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        decode_mla(q, kn, kr, out, lens, 576 ** -0.5, page, bt, plan=plan)
    own = torch.empty_like(out)
    for new in (torch.full((B,), 1024), torch.full((B,), 4096), torch.full((B,), 1), torch.arange(B) * 256 + 1,
                torch.full((B,), 2048 + 31), torch.full((B,), 2048 - 33), torch.full((B,), 2048)):
        lens.copy_(new.to(torch.int32).cuda())
        out.fill_(3.0)
        graph.replay()
        torch.ops.npu.decode_mla(q, kn, kr, own, lens, 576 ** -0.5, page, bt, -1)
        torch.cuda.synchronize()
        assert torch.allclose(out.float(), own.float(), rtol=2 ** -7, atol=2e-3), (int(new[0]), (out.float() - own.float()).abs().max())


def _pair_inputs(B, Hq, S, page, dtype, ragged, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    maxp = (S + page - 1) // page
    nb = B * maxp
    q = torch.randn((B, Hq, 576), generator=g, device="cuda").to(dtype)
    kn = (torch.randn((nb, page, 1, 512), generator=g, device="cuda") * 0.5).to(dtype)
    kr = (torch.randn((nb, page, 1, 64), generator=g, device="cuda") * 0.5).to(dtype)
    bt = torch.randperm(nb, generator=g, device="cuda").to(torch.int32).reshape(B, maxp)
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    if ragged:
        lens = torch.randint(1, S + 1, (B,), generator=g, device="cuda").to(torch.int32)
    return q, kn, kr, lens, bt


# B, Hq, S, page, dtype, ragged, num_splits -- batches the list (or num_splits = 2) cuts into two pieces per sequence: BASELINE C4's shape
# at a quarter of its length, a ragged copy (sequences of one, two and three pieces side by side: uneven arrival), a partly filled head
# block in fp16, the uniform two-split form on a small batch, pages of 32 keys
PAIR_CASES = [(128, 128, 1024, 64, torch.bfloat16, False, PLANNED), (128, 128, 1500, 64, torch.bfloat16, True, PLANNED),
              (100, 96, 700, 128, torch.float16, True, PLANNED), (5, 128, 900, 64, torch.bfloat16, True, 2),
              (120, 128, 640, 32, torch.float16, False, PLANNED),
              # more workgroups than CUs: 200 sequences x two uniform splits = 400 workgroups (a piece may meet a partner that is not
              # resident yet: the bounded wait, then the merge kernel -- or simply a late partner), and the list form of the same batch
              (200, 128, 700, 64, torch.bfloat16, True, 2), (200, 128, 1100, 64, torch.bfloat16, True, PLANNED)]


@pytest.mark.parametrize("B,Hq,S,page,dtype,ragged,splits", PAIR_CASES)
def test_two_piece_sequences_finish_between_their_workgroups(B, Hq, S, page, dtype, ragged, splits):
    """Sequences in two pieces finish inside the kernel (each workgroup: one half of the output dimensions, mla_decode_wide8s.hip);
    the same sums in the same order as the merge kernel, so the outputs are THE BITS of the run with the pair finish off -- also when
    the second piece withholds its word and the first runs into its bounded wait (mode 2: the merge kernel does the work), and over
    repeated calls on one workspace (the meeting words are re-armed by the merge kernel)."""
    L = lib()
    L.mi_mla_decode_set_pair.argtypes = [c_int]
    q, kn, kr, lens, bt = _pair_inputs(B, Hq, S, page, dtype, ragged, 5)
    sm = 576 ** -0.5
    try:
        assert L.mi_mla_decode_select_wide(9) == 0
        assert L.mi_mla_decode_set_pair(0) == 0
        want = run_mla(q, kn, kr, lens, bt, sm, splits)
        assert L.mi_mla_decode_set_pair(1) == 0
        keep = []
        got = run_mla(q, kn, kr, lens, bt, sm, splits, keep_ws=keep)
        assert torch.equal(got, want), (got.float() - want.float()).abs().max()
        # the same workspace again and again (words re-armed), with other queries in between
        ws = keep[0]
        for rep in range(3):
            q2 = (q.float() * (1.0 + 0.25 * rep)).to(dtype)
            L.mi_mla_decode_set_pair(0)
            want2 = run_mla(q2, kn, kr, lens, bt, sm, splits)
            L.mi_mla_decode_set_pair(1)
            out = torch.empty_like(want2)
            rc = L.mi_mla_decode(ptr(q2), ptr(kn), ptr(kr), ptr(out), ptr(lens), ptr(bt), B, Hq, 1, page, bt.stride(0), S, q2.stride(0), q2.stride(1),
                                 kn.stride(0), kn.stride(1), kn.stride(2), kr.stride(0), kr.stride(1), kr.stride(2), out.stride(0), out.stride(1),
                                 sm, 0 if dtype == torch.bfloat16 else 1, splits, ptr(ws), ws.numel(), stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(out, want2), rep
        assert L.mi_mla_decode_set_pair(2) == 0
        got = run_mla(q, kn, kr, lens, bt, sm, splits)
        assert torch.equal(got, want), "bounded wait -> merge kernel"
        # ... and the words a timed-out call left behind do not leak into the next one
        assert L.mi_mla_decode_set_pair(1) == 0
        got = run_mla(q, kn, kr, lens, bt, sm, splits)
        assert torch.equal(got, want)
    finally:
        L.mi_mla_decode_set_pair(-1)
        L.mi_mla_decode_select_wide(0)


def test_pair_finish_in_a_replayed_graph():
    """The pair finish inside a captured graph: every replay carries the same tag, the meeting words are re-armed by the merge kernel
    of the replay before -- outputs follow the inputs written between replays, bit for bit the eager result with the pair finish off."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgl-kernel-npu_amd", "python"))
    from sgl_kernel_npu.attention.decode_attention import decode_mla, decode_mla_plan
    L = lib()
    L.mi_mla_decode_set_pair.argtypes = [c_int]
    B, Hq, S, page = 128, 128, 1024, 64
    q, kn, kr, lens, bt = _pair_inputs(B, Hq, S, page, torch.bfloat16, False, 11)
    out = torch.empty((B, Hq, 512), dtype=torch.bfloat16, device="cuda")
    plan = decode_mla_plan(lens, 1)
    try:
        L.mi_mla_decode_set_pair(1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            decode_mla(q, kn, kr, out, lens, 576 ** -0.5, page, bt, plan=plan)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            decode_mla(q, kn, kr, out, lens, 576 ** -0.5, page, bt, plan=plan)
        for rep in range(4):
            q.copy_((torch.randn(q.shape, device="cuda") * (1 + rep)).to(torch.bfloat16))
            out.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            L.mi_mla_decode_set_pair(0)
            want = torch.empty_like(out)
            decode_mla(q, kn, kr, want, lens, 576 ** -0.5, page, bt, plan=plan)
            torch.cuda.synchronize()
            L.mi_mla_decode_set_pair(1)
            assert torch.equal(got, want), rep
    finally:
        L.mi_mla_decode_set_pair(-1)
