"""GPU: torch.ops.npu.compressor (csrc/kernels/compressor.hip) against the float64 restatement of tests/compressor_ref.py: the stored cases of
the reference test's golden and its other small cases, ragged batches, the K-loop tail and a long K loop, both GEMM forms and the row count
between them, both rotary modes and dtypes, a paged table with a 0 entry, BSH against TH, chained calls that thread one state_cache, graph
replay and run-to-run identity.  Every state row a call neither reads nor writes holds NaN.

Bounds (the issue's, derived there; not tuned): every filled cmp_kv element within 1 ulp of the output dtype taken at max(|ref64|, 2^-6);
unfilled rows are zeros; a written state row within H 2^-24 sum_k |x_k w_k| (+ 2^-24 |ape| on the score half); every other state row
bit-identical."""
import numpy as np
import pytest
import torch

import compressor_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16 = torch.bfloat16, torch.float16
_REFS = {}


def _op():
    import sgl_kernel_npu  # noqa: F401

    return torch.ops.npu.compressor


def reference(c):
    """The float64 restatement of a case, computed once per case name and left unchanged."""
    if c["name"] not in _REFS:
        _REFS[c["name"]] = R.compress_ref(c, round_out=False)
    return _REFS[c["name"]]


def on_gpu(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def run(g, **over):
    """-> cmp_kv; g["state_cache"] is updated in place."""
    kw = dict(state_block_table=g["state_block_table"], cu_seqlens=g["cu_seqlens"], seqused=g["seqused"], start_pos=g["start_pos"],
              rope_head_dim=64, cmp_ratio=g["r"], coff=g["coff"], norm_eps=g["norm_eps"], rotary_mode=g["rotary_mode"],
              cache_mode=g["cache_mode"], state_cache_stride_dim0=0)
    kw.update(over)
    return _op()(g["x"], g["wkv"], g["wgate"], g["state_cache"], g["ape"], g["norm_weight"], g["rope_sin"], g["rope_cos"], **kw)


def check(c, out, state, what, ref=None):
    """out, state: what the kernel left, on any device."""
    ref = ref or reference(c)
    ww2 = 2 * c["coff"] * c["D"]
    got = out.detach().cpu().double().numpy().reshape(-1, c["D"])
    f = ref["filled"]
    assert got.shape[0] == len(f) and out.dtype == c["dtype"]
    assert not np.isnan(got).any(), f"{what}: NaN in cmp_kv (a poisoned state row was read)"
    assert not got[~f].any(), f"{what}: a row no group fills is not zero"
    if f.any():
        err = np.abs(got[f] - ref["cmp_kv"][f]) / R.ulp_bound(ref["cmp_kv"][f], c["dtype"])
        print(what, "filled rows", int(f.sum()), "max |cmp_kv - ref64| in ulp at max(|ref64|, 2^-6):", float(err.max()))
        assert err.max() <= 1.0, what
    after = state.detach().cpu().reshape(-1, ww2)
    before = c["state_cache"].reshape(-1, ww2)
    keep = torch.from_numpy(~ref["written"])
    assert torch.equal(after[keep].view(torch.int32), before[keep].view(torch.int32)), f"{what}: a state row the call must not write changed"
    worst = 0.0
    for row, lim in R.state_bound(c, ref).items():
        err = np.abs(after[row].double().numpy() - ref["state"][row])
        assert (err <= lim).all(), f"{what}: state row {row}"
        worst = max(worst, float((err / lim).max()))
    print(what, "written state rows", int(ref["written"].sum()), "max |state - ref64| / bound:", worst)


def run_and_check(c, what=None):
    g = on_gpu(c)
    out = run(g)
    torch.cuda.synchronize()
    check(c, out, g["state_cache"], what or c["name"])
    return out, g


# ---- 1. the stored cases (also held to the stored golden itself) and the reference test's other small cases
@pytest.mark.parametrize("path", R.golden_paths(), ids=lambda p: p.split("_")[-1][:1])
def test_stored_reference_cases(path):
    c, z = R.load_golden(path)
    out, g = run_and_check(c)
    f = z["filled"]
    golden = torch.from_numpy(z["cmp_kv_bits"]).view(c["dtype"]).double().numpy()
    ref = reference(c)["cmp_kv"]
    # the golden and the kernel are each within 1 ulp of ref64
    assert (np.abs(out.cpu().double().numpy()[f] - golden[f]) <= 2 * R.ulp_bound(ref[f], c["dtype"])).all()
    stride = int(z["state_stride"])
    after = g["state_cache"].cpu().reshape(-1, 2 * c["coff"] * c["D"]).double().numpy()
    sb = R.state_bound(c, reference(c))
    for row, vals in zip(z["state_rows"], z["state_values"]):
        assert (np.abs(after[row][::stride] - vals) <= 2 * sb[int(row)][::stride]).all()


SMALL = {
    "ring_c128a_sp300": dict(shape="c128a", starts=[300], spans=[129], cache_mode=2, seed=11),
    "ring_two_sequences": dict(shape="c128a", starts=[200, 328], spans=[129, 129], cache_mode=2, seed=12),
    "paged_two_sequences": dict(shape="c4a", starts=[0, 128], spans=[128, 128], cache_mode=1, seed=13),
    # 2. ragged: a sequence that completes no group (1), a one-token sequence that completes a group from saved state (2), one that does
    # not (3), seqused below the span (0)
    "ragged_paged": dict(shape="c4a", starts=[5, 0, 131, 128], spans=[70, 3, 1, 1], seqused=[66, 3, 1, 1], cache_mode=1, seed=21),
    "ragged_ring": dict(shape="c4li", starts=[5, 0, 131, 128], spans=[70, 3, 1, 1], seqused=[66, 3, 1, 1], cache_mode=2, seed=22, dtype=FP16),
    # 3. the K-loop tail (1536 = 24 k-tiles, no power of two) and a long K loop
    "h1536": dict(shape="c4a", starts=[3], spans=[5], cache_mode=1, seed=31, H=1536),
    "h7168": dict(shape="c128a", starts=[125], spans=[5], cache_mode=2, seed=32, H=7168, dtype=FP16),
    # 4. T = 1, 129 (two M tiles of the skinny form), 256 / 257 (either side of the form switch), 300 (two sequences meet inside an M tile)
    "t1": dict(shape="c4a", starts=[7], spans=[1], cache_mode=1, seed=41),
    "t129": dict(shape="c4li", starts=[2], spans=[129], cache_mode=2, seed=42),
    "t256": dict(shape="c4li", starts=[1, 9], spans=[250, 6], cache_mode=1, seed=43, dtype=FP16),
    "t257": dict(shape="c4li", starts=[1, 9], spans=[250, 7], cache_mode=1, seed=44),
    "t257_fp16": dict(shape="c4a", starts=[1, 9], spans=[250, 7], cache_mode=2, seed=46, dtype=FP16),
    "t300": dict(shape="c128a", starts=[60, 0], spans=[100, 200], cache_mode=1, seed=45),
    # 5. rotary modes and dtypes
    "half_bf16": dict(shape="c4a", starts=[13], spans=[9], cache_mode=1, seed=51, rotary_mode=1),
    "half_fp16": dict(shape="c128a", starts=[120], spans=[9], cache_mode=2, seed=52, rotary_mode=1, dtype=FP16),
    "interleave_fp16": dict(shape="c4li", starts=[13], spans=[9], cache_mode=2, seed=53, rotary_mode=2, dtype=FP16),
}


def small_case(name):
    kw = dict(SMALL[name])
    return R.make_case(name, kw.pop("shape"), kw.pop("starts"), kw.pop("spans"), kw.pop("cache_mode"), **kw)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_cases(name):
    c = small_case(name)
    ref = reference(c)
    assert ref["filled"].any() and ref["written"].any()
    assert torch.isnan(c["state_cache"]).any()
    if name.startswith("ragged"):
        tokens, _, slots = R.plan(c)
        per_seq = [sum(1 for s in slots if s[1] == b) for b in range(4)]
        assert per_seq[1] == 0 and per_seq[2] == 1 and per_seq[3] == 0 and len([t for t in tokens if t[1] == 0]) == 66
        assert all(kind == "state" for s in slots if s[1] == 2 for _, kind, _ in s[3][:-1])
    run_and_check(c)


# ---- 6. a paged table with a 0 entry in the middle of a sequence
def test_zero_table_entry_is_read_but_never_written():
    c = R.make_case("zero_entry", "c4a", [20], [40], 1, seed=61, zero_entries=[(0, 2)])      # positions 32..47 map to block 0
    ref = reference(c)
    _, saves, slots = R.plan(c)
    assert len(saves) == 40 - 16 and not ref["written"][:16].any()
    c2 = R.make_case("zero_entry_history", "c4a", [36], [9], 1, seed=62, zero_entries=[(0, 2)])      # history 28..35 reaches into block 0
    assert reference(c2)["read"][:16].any()
    for case in (c, c2):
        before = case["state_cache"][0].clone()
        _, g = run_and_check(case)
        assert torch.equal(g["state_cache"][0].cpu().view(torch.int32), before.view(torch.int32))


# ---- 7. BSH equals TH on the same tokens
@pytest.mark.parametrize("mode", [1, 2])
def test_bsh_equals_th(mode):
    kw = dict(seed=71, seqused=[9, 12, 5])
    th = R.make_case(f"th_{mode}", "c4a", [13, 0, 6], [12, 12, 12], mode, **kw)
    bsh = R.make_case(f"bsh_{mode}", "c4a", [13, 0, 6], [12, 12, 12], mode, layout="BSH", **kw)
    cg = 3
    assert torch.equal(th["x"], bsh["x"].view(36, -1)) and torch.equal(th["state_cache"].view(torch.int32), bsh["state_cache"].view(torch.int32))
    # rope rows travel with the group: TH packs them, BSH keeps [b, j]
    _, _, slots = R.plan(bsh)
    packed = [s[0] for s in slots]
    assert packed != list(range(len(packed)))                                    # the mapping is not the identity
    for i, o in enumerate(packed):
        bsh["rope_sin"].view(-1, 64)[o] = th["rope_sin"][i]
        bsh["rope_cos"].view(-1, 64)[o] = th["rope_cos"][i]
    out_th, g_th = run_and_check(th)
    out_bsh, g_bsh = run_and_check(bsh)
    assert out_bsh.shape == (3, cg, 512)
    assert torch.equal(out_bsh.view(-1, 512)[packed].view(torch.int16), out_th[:len(packed)].view(torch.int16))
    assert torch.equal(g_th["state_cache"].view(torch.int32), g_bsh["state_cache"].view(torch.int32))


# ---- 8. chaining: the state semantics
@pytest.mark.parametrize("mode", [1, 2], ids=["paged", "ring"])
@pytest.mark.parametrize("shape,start", [("c4a", 0), ("c128a", 0), ("c128a", 116)])
def test_chained_calls_equal_one_call(shape, start, mode):
    r, coff, _ = R.SHAPES[shape]
    total, pieces = 23, (9, 1, 1, 5, 7)
    ring = max(16, coff * r + total - 1)                                         # the reference test's ring for the single call
    name = f"chain_{shape}_{start}_{mode}"
    one = R.make_case(name, shape, [start], [total], mode, seed=81, ring=ring, poison=False)
    ref_one = reference(one)
    out_one, g_one = run_and_check(one)
    state = one["state_cache"]
    rows, done, at = [], 0, 0
    for n in pieces:
        c = R.make_case(f"{name}_{at}", shape, [start + at], [n], mode, seed=81, ring=ring, state=state, table=one["state_block_table"] if mode == 1 else None)
        c.update(x=one["x"][at:at + n], wkv=one["wkv"], wgate=one["wgate"], ape=one["ape"], norm_weight=one["norm_weight"])
        groups = (start + at + n) // r - (start + at) // r
        c["rope_sin"][:groups], c["rope_cos"][:groups] = one["rope_sin"][done:done + groups], one["rope_cos"][done:done + groups]
        out, g = run_and_check(c)
        assert int(reference(c)["filled"].sum()) == groups
        rows.append(out[:groups].cpu())
        state = g["state_cache"].cpu()
        done, at = done + groups, at + n
    assert at == total and done == int(ref_one["filled"].sum())
    if done:
        chained = torch.cat(rows).double().numpy()
        f = ref_one["filled"]
        err = np.abs(chained - ref_one["cmp_kv"][f]) / R.ulp_bound(ref_one["cmp_kv"][f], one["dtype"])
        print(name, "chained rows against the single call's ref64, ulp:", float(err.max()))
        assert err.max() <= 1.0
    # the state rows the single call wrote hold the same values after the chain
    ww2 = 2 * coff * R.SHAPES[shape][2]
    a, b = state.reshape(-1, ww2)[torch.from_numpy(ref_one["written"])].double().numpy(), ref_one["state"][ref_one["written"]]
    lim = np.stack([v for _, v in sorted(R.state_bound(one, ref_one).items())])
    assert (np.abs(a - b) <= lim).all()


# ---- 9. graph capture without a warm-up, replays after the inputs changed in place
def test_graph_replay_reads_the_current_inputs():
    spans = [9, 7]
    cases = [R.make_case(f"graph_{i}", "c4a", st, spans, 1, seed=90 + i, seqused=su)
             for i, (st, su) in enumerate((([13, 2], [9, 7]), ([20, 16], [5, 7]), ([4, 25], [9, 3])))]
    assert len({tuple(c["state_block_table"].shape) for c in cases}) == 1 and len({tuple(c["state_cache"].shape) for c in cases}) == 1
    g = on_gpu(cases[0])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        out = run(g)
    torch.cuda.synchronize()
    keys = ("x", "start_pos", "seqused", "state_cache", "state_block_table", "rope_sin", "rope_cos", "ape", "wkv", "wgate", "norm_weight")
    for c in cases:
        for k in keys:
            g[k].copy_(c[k].to(DEV))                                             # in place: the captured launches see the same storage
        graph.replay()
        torch.cuda.synchronize()
        check(c, out, g["state_cache"], f"replay {c['name']} start {c['start_pos'].tolist()} used {c['seqused'].tolist()}")


# ---- 10. run-to-run identity (the K split adds slabs in a fixed order)
@pytest.mark.parametrize("name", ["h7168", "t300", "ragged_paged"])
def test_two_runs_give_the_same_bits(name):
    c = small_case(name)
    a, b = on_gpu(c), on_gpu(c)
    out_a, out_b = run(a), run(b)
    torch.cuda.synchronize()
    assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16))
    assert torch.equal(a["state_cache"].view(torch.int32), b["state_cache"].view(torch.int32))


# ---- defaults and refusals of the op
def test_defaults_and_refusals():
    c = R.make_case("defaults", "c4a", [0, 0], [8, 8], 1, seed=95, layout="BSH")
    g = on_gpu(c)
    out = run(g, seqused=None, start_pos=None)                                   # None: the whole span, from position 0
    torch.cuda.synchronize()
    check(c, out, g["state_cache"], "seqused = start_pos = None")
    th = R.make_case("refuse_th", "c4a", [13], [9], 1, seed=96)
    t = on_gpu(th)
    canary = t["state_cache"].clone()
    bad = [
        (dict(cu_seqlens=None), "cu_seqlens should not be None"), (dict(cmp_ratio=8), "cmpRatio"), (dict(coff=1), "coff"),
        (dict(rope_head_dim=32), "ropeHeadDim"), (dict(rotary_mode=3), "mi_compressor failed"), (dict(cache_mode=0), "mi_compressor failed"),
        (dict(state_cache_stride_dim0=5), "mi_compressor failed"), (dict(seqused=torch.zeros(2, dtype=torch.int32, device=DEV)), "seqused"),
        (dict(start_pos=t["start_pos"].long()), "int32"), (dict(state_block_table=None), "state_block_table"),
        (dict(state_block_table=t["state_block_table"][:, 0].contiguous(), cache_mode=2), "mi_compressor failed"),      # explicit mode wants a 2-D table
    ]
    for over, text in bad:
        with pytest.raises(RuntimeError, match=text):
            run(t, **over)
    with pytest.raises(RuntimeError, match="must be None"):
        run(g, cu_seqlens=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="hidden"):
        run(dict(t, x=t["x"][:, :512].contiguous(), wkv=t["wkv"][:, :512].contiguous(), wgate=t["wgate"][:, :512].contiguous()))
    torch.cuda.synchronize()
    assert torch.equal(canary.view(torch.int32), t["state_cache"].view(torch.int32))
    # T = 0: the empty output, no launch
    out = run(dict(t, x=t["x"][:0], rope_sin=t["rope_sin"][:0], rope_cos=t["rope_cos"][:0], cu_seqlens=torch.zeros(2, dtype=torch.int32, device=DEV)))
    assert out.shape == (0, 512) and out.dtype == BF16
