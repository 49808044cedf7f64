"""float64 restatement of torch.ops.npu.compressor (include/mi_sgl_kernels.h) and the case maker of its tests.

Token i < used_b of sequence b stands at position pos = start_b + i.  kv = x . wkv^T, score = x . wgate^T + ape[pos % r].  A group of r
positions that ends inside the call (group start < ((start + used) // r) * r) becomes one output row: its rows, channels [(coff - 1) D, coff D),
stacked behind -- coff = 2 -- the previous group's rows, channels [0, D); a row is this call's projection where pos >= start, a state_cache
row where it is before, (0, -inf) before position 0; softmax over the stacked rows per channel, weighted sum of kv, RMSNorm, RoPE on the last
64 channels, one rounding to x's dtype.  State rows are READ as they were before the call and written afterwards: paged (cache_mode 1) every
token unless its table entry is 0, explicit (cache_mode 2) the tokens of groups that start at or behind the last complete group boundary
minus (coff - 1) r.

Every input is drawn from numpy.random.default_rng(seed).integers(...) and scaled onto a grid that bf16 and fp16 hold exactly, so a case is
rebuilt from its seed and parameters.  Every state_cache row the call neither reads nor writes holds NaN."""
import functools
import glob
import json
import os
import zlib

import numpy as np
import torch

DTYPES = (torch.bfloat16, torch.float16)
ROPE = 64
SHAPES = {"c4a": (4, 2, 512), "c4li": (4, 2, 128), "c128a": (128, 1, 512)}      # (cmp_ratio, coff, head_dim)
INPUTS = ("x", "wkv", "wgate", "ape", "norm_weight", "rope_sin", "rope_cos", "state_cache", "state_block_table", "start_pos", "seqused")


def ulp_bound(want, dtype):
    """1 ulp of the output dtype, taken at max(|want|, 2^-6)."""
    bits = 7 if dtype == torch.bfloat16 else 10
    mag = np.maximum(np.abs(want), 2.0 ** -6)
    return 2.0 ** (np.floor(np.log2(mag)) - bits)


def out_rows(c):
    T, B, r = c["tokens"], len(c["spans"]), c["r"]
    return min(T, T // r + B) if c["layout"] == "TH" else B * (-(-c["S"] // r))


def plan(c):
    """Index pass.  -> tokens [(row, b, pos)], saves {token row: flat state row}, slots [(out row, b, group start, sources)] with sources
    [(part, 'new', token row) | (part, 'state', flat state row) | (part, 'none', 0)] in stacking order."""
    r, coff, mode, bs = c["r"], c["coff"], c["cache_mode"], c["block_size"]
    table = c["state_block_table"].numpy()
    th = c["layout"] == "TH"
    cg = 0 if th else -(-c["S"] // r)

    def loc(b, pos, start):
        if mode == 1:
            return int(table[b, pos // bs]) * bs + pos % bs
        return int(table[b, coff * r + pos - start])

    tokens, saves, slots, packed, base = [], {}, [], 0, 0
    for b, span in enumerate(c["spans"]):
        start, used = int(c["start_pos"][b]), int(c["seqused"][b]) if c.get("seqused") is not None else span
        done = (start + used) // r * r
        for i in range(used):
            pos = start + i
            tokens.append((base + i, b, pos))
            if mode == 1:
                if int(table[b, pos // bs]) != 0:
                    saves[base + i] = loc(b, pos, start)
            elif pos // r * r >= done - (coff - 1) * r:
                saves[base + i] = loc(b, pos, start)
        for j in range(((start + used) // r - start // r) if used > 0 else 0):
            gs = (start // r + j) * r
            src = []
            for part in range(coff):
                for pos in range(gs - (coff - 1 - part) * r, gs - (coff - 1 - part) * r + r):
                    if pos < 0:
                        src.append((part, "none", 0))
                    elif pos >= start:
                        src.append((part, "new", base + pos - start))
                    else:
                        src.append((part, "state", loc(b, pos, start)))
            slots.append((packed if th else b * cg + j, b, gs, src))
            packed += 1
        base += span
    return tokens, saves, slots


def rope_ref(v, sin, cos, mode):
    y = v.copy()
    if mode == 1:
        a, b = v[:32], v[32:]
        y[:32] = a * cos[:32] - b * sin[:32]
        y[32:] = a * sin[32:] + b * cos[32:]
    else:
        a, b = v[0::2], v[1::2]
        y[0::2] = a * cos[0::2] - b * sin[0::2]
        y[1::2] = a * sin[1::2] + b * cos[1::2]
    return y


def compress_ref(c, compute=np.float64, round_out=True):
    """-> dict(cmp_kv [out rows, D] (rounded once to the case's dtype unless round_out is off), filled [out rows] bool, state [rows, 2 ww]
    after the call, written [rows] bool, read [rows] bool, absdot [T, 2 ww] = sum_k |x_k w_k| (the scale of the state bound))."""
    r, coff, D, ww = c["r"], c["coff"], c["D"], c["coff"] * c["D"]
    f = lambda t: t.to(torch.float64).numpy().astype(compute)      # noqa: E731
    x = f(c["x"]).reshape(-1, c["H"])
    wkv, wgate, ape, nw = f(c["wkv"]), f(c["wgate"]), f(c["ape"]), f(c["norm_weight"])
    sin, cos = f(c["rope_sin"]).reshape(-1, ROPE), f(c["rope_cos"]).reshape(-1, ROPE)
    state = f(c["state_cache"]).reshape(-1, 2 * ww)
    tokens, saves, slots = plan(c)
    new = np.concatenate([x @ wkv.T, x @ wgate.T], axis=1)
    for row, _, pos in tokens:
        new[row, ww:] += ape[pos % r]
    n_out = out_rows(c)
    out, filled = np.zeros((n_out, D), dtype=compute), np.zeros(n_out, dtype=bool)
    read = np.zeros(state.shape[0], dtype=bool)
    for o, b, gs, src in slots:
        K, S = np.zeros((coff * r, D), dtype=compute), np.full((coff * r, D), -np.inf, dtype=compute)
        for n, (part, kind, row) in enumerate(src):
            if kind == "none":
                continue
            rows = new if kind == "new" else state
            K[n], S[n] = rows[row, part * D:(part + 1) * D], rows[row, ww + part * D:ww + (part + 1) * D]
            if kind == "state":
                read[row] = True
        e = np.exp(S - S.max(axis=0, keepdims=True))
        v = (K * (e / e.sum(axis=0, keepdims=True))).sum(axis=0)
        v = nw * (v * (1.0 / np.sqrt(np.mean(np.square(v)) + compute(c["norm_eps"]))))
        v[-ROPE:] = rope_ref(v[-ROPE:], sin[o], cos[o], c["rotary_mode"])
        out[o], filled[o] = v, True
    after, written = state.copy(), np.zeros(state.shape[0], dtype=bool)
    for row, dst in saves.items():
        after[dst], written[dst] = new[row], True
    if round_out:
        out = torch.from_numpy(out.astype(np.float64)).to(c["dtype"]).to(torch.float64).numpy()
    absdot = np.concatenate([np.abs(x) @ np.abs(wkv).T, np.abs(x) @ np.abs(wgate).T], axis=1)
    return dict(cmp_kv=out, filled=filled, state=after, written=written, read=read, absdot=absdot)


def state_bound(c, ref, rows=None):
    """|state - ref64| <= H 2^-24 sum_k |x_k w_k| (+ 2^-24 |ape| on the score half) per written flat state row -> {state row: [2 ww]}."""
    ww = c["coff"] * c["D"]
    tokens, saves, _ = plan(c)
    pos_of = {row: pos for row, _, pos in tokens}
    ape = c["ape"].double().numpy()
    out = {}
    for row, dst in saves.items():
        bound = c["H"] * 2.0 ** -24 * ref["absdot"][row]
        bound[ww:] += 2.0 ** -24 * np.abs(ape[pos_of[row] % c["r"]])
        out[dst] = bound
    return out


def make_case(name, shape, starts, spans, cache_mode, dtype=torch.bfloat16, seed=0, H=1024, seqused=None, block_size=16, rotary_mode=2,
              layout="TH", zero_entries=(), ring=None, state=None, table=None, poison=True):
    """shape: a key of SHAPES.  Paged: a shuffled table of distinct blocks >= 1 (zero_entries: (b, column) pairs set to 0; block 0 exists).
    Explicit: the reference test's ring, one bank per sequence of `ring` slots (default max(block_size, coff r + longest span - 1): the
    oldest history position and the newest token share a slot), loc = b * ring + pos % ring, columns of negative positions -> a spare row.
    state / table: a state_cache (then nothing is poisoned) and a paged table to thread through a chain of calls instead of drawn ones."""
    r, coff, D = SHAPES[shape]
    ww, B = coff * D, len(starts)
    rng = np.random.default_rng(seed)
    T = sum(spans)
    S = spans[0] if layout == "BSH" else 0
    assert layout == "TH" or all(s == S for s in spans)
    grid = lambda shp, lo, hi, scale: torch.from_numpy(rng.integers(lo, hi + 1, size=shp).astype(np.float64) * scale)      # noqa: E731
    c = dict(name=name, shape=shape, r=r, coff=coff, D=D, H=H, cache_mode=cache_mode, dtype=dtype, seed=seed, layout=layout, spans=list(spans),
             S=S, tokens=T, rotary_mode=rotary_mode, norm_eps=1e-6, start_pos=torch.tensor(starts, dtype=torch.int32),
             seqused=torch.tensor(seqused, dtype=torch.int32) if seqused is not None else None)
    c["x"] = grid((T, H), -8, 8, 2.0 ** -8).to(dtype)
    if layout == "BSH":
        c["x"] = c["x"].view(B, S, H)
    c["wkv"] = grid((ww, H), -8, 8, 2.0 ** -8).to(dtype)
    c["wgate"] = grid((ww, H), -8, 8, 2.0 ** -3).to(dtype)
    c["ape"] = grid((r, ww), -16, 16, 2.0 ** -6).float()
    c["norm_weight"] = (1.0 + grid((D,), -2, 2, 2.0 ** -6)).float()
    c["cu_seqlens"] = torch.tensor(np.concatenate([[0], np.cumsum(spans)]), dtype=torch.int32) if layout == "TH" else None
    ends = [s + n for s, n in zip(starts, spans)]
    if cache_mode == 1:
        cols = table.shape[1] if table is not None else max(-(-e // block_size) for e in ends)
        blocks = 1 + B * cols + 1
        drawn_table = torch.from_numpy(1 + rng.permutation(B * cols).reshape(B, cols).astype(np.int32))
        c["state_block_table"] = drawn_table if table is None else table.clone()
        for b, col in zero_entries:
            c["state_block_table"][b, col] = 0
        c["block_size"] = block_size
    else:
        hist = coff * r
        size = ring or max(block_size, hist + max(spans) - 1)
        blocks = B + 1
        table = np.full((B, hist + max(spans)), B * size, dtype=np.int32)
        for b in range(B):
            for col in range(hist + spans[b]):
                pos = starts[b] - hist + col
                if pos >= 0:
                    table[b, col] = b * size + pos % size
        c["state_block_table"] = torch.from_numpy(table)
        c["block_size"] = size
    drawn = torch.cat([grid((blocks, c["block_size"], ww), -16, 16, 2.0 ** -10), grid((blocks, c["block_size"], ww), -16, 16, 2.0 ** -4)], dim=2).float()
    c["state_cache"] = drawn if state is None else state.clone()
    n_out = out_rows(c)      # drawn last: the row count depends on the layout, nothing else does
    c["rope_sin"] = grid((n_out, ROPE), -64, 64, 2.0 ** -7).float()
    c["rope_cos"] = (1.0 + grid((n_out, ROPE), -64, 64, 2.0 ** -7)).float()
    if layout == "BSH":
        c["rope_sin"], c["rope_cos"] = c["rope_sin"].view(B, -1, ROPE), c["rope_cos"].view(B, -1, ROPE)
    if poison and state is None:
        _, saves, slots = plan(c)
        keep = np.zeros(blocks * c["block_size"], dtype=bool)
        keep[list(saves.values())] = True
        for _, _, _, src in slots:
            for _, kind, row in src:
                if kind == "state":
                    keep[row] = True
        c["state_cache"].view(-1, 2 * ww)[torch.from_numpy(~keep)] = float("nan")
    return c


def checksums(c):
    """crc32 of every input's bytes, in INPUTS order (seqused absent: 0)."""
    def crc(t):
        if t is None:
            return 0
        a = t.contiguous()
        a = a.view(torch.int16) if a.dtype in DTYPES else a
        return zlib.crc32(a.numpy().tobytes())
    return np.array([crc(c.get(k)) for k in INPUTS], dtype=np.int64)


# ---- the stored cases of the reference test's golden (tests/golden/gen_compressor_golden.py writes them)
GOLDEN_CASES = [
    dict(name="a", shape="c4li", starts=[13], spans=[9], cache_mode=2, dtype="bfloat16", seed=600),
    dict(name="b", shape="c4li", starts=[13], spans=[9], cache_mode=1, dtype="float16", seed=601),
    dict(name="c", shape="c4a", starts=[13], spans=[9], cache_mode=2, dtype="float16", seed=602),
    dict(name="d", shape="c4a", starts=[13], spans=[9], cache_mode=1, dtype="bfloat16", seed=603),
    dict(name="e", shape="c128a", starts=[200], spans=[129], cache_mode=2, dtype="bfloat16", seed=604),
    dict(name="f", shape="c128a", starts=[200], spans=[129], cache_mode=1, dtype="float16", seed=605),
    dict(name="g", shape="c128a", starts=[0], spans=[129], cache_mode=2, dtype="bfloat16", seed=606),
    dict(name="h", shape="c4a", starts=[5, 0, 18], spans=[11, 3, 6], cache_mode=1, dtype="bfloat16", seed=607, rotary_mode=1),
]


def golden_case(spec):
    kw = dict(spec)
    kw["dtype"] = getattr(torch, kw["dtype"])
    name = kw.pop("name")
    return make_case("golden_" + name, kw.pop("shape"), kw.pop("starts"), kw.pop("spans"), kw.pop("cache_mode"), **kw)


def golden_paths():
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compressor_ref_*.npz")))


def load_golden(path):
    """-> (the case rebuilt from the stored seed and parameters, the stored arrays)."""
    z = np.load(path)
    spec = json.loads(str(z["spec"]))
    c = golden_case(spec)
    assert np.array_equal(checksums(c), z["checksums"]), f"{path}: the rebuilt inputs differ from the ones the golden ran on"
    return c, {k: z[k] for k in z.files}


# ---- the C-ABI's parameter block (include/mi_sgl_kernels.h: mi_compressor_params)
@functools.lru_cache(maxsize=None)
def params_type():
    import ctypes as C

    class Params(C.Structure):
        _fields_ = ([(n, C.c_void_p) for n in ("x", "wkv", "wgate", "state_cache", "ape", "norm_weight", "rope_sin", "rope_cos",
                                               "state_block_table", "cu_seqlens", "seqused", "start_pos", "cmp_kv", "workspace")] +
                    [("workspace_bytes", C.c_size_t)] +
                    [(n, C.c_int64) for n in ("tokens", "out_rows", "state_blocks", "table_stride", "state_cache_stride_dim0")] +
                    [(n, C.c_int) for n in ("layout", "batch", "seq", "hidden", "head_dim", "cmp_ratio", "coff", "rope_head_dim", "rotary_mode",
                                            "cache_mode", "block_size", "table_dims", "table_cols", "dtype")] +
                    [("norm_eps", C.c_float)])
    return Params


def bind(lib):
    import ctypes as C

    lib.mi_compressor_workspace.restype = C.c_size_t
    lib.mi_compressor_workspace.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.mi_compressor.restype = C.c_int
    lib.mi_compressor.argtypes = [C.POINTER(params_type()), C.c_void_p]
    return lib


def fill_params(c, pointers, **over):
    """The parameter block of case c; pointers: name -> address (or a tensor-free dummy), over: fields to overwrite."""
    P = params_type()
    B = len(c["spans"])
    table = c["state_block_table"]
    p = P(tokens=c["tokens"], out_rows=out_rows(c), state_blocks=c["state_cache"].shape[0], table_stride=table.shape[1] if table.dim() == 2 else 1,
          state_cache_stride_dim0=0, layout=0 if c["layout"] == "TH" else 1, batch=B, seq=c["S"], hidden=c["H"], head_dim=c["D"], cmp_ratio=c["r"],
          coff=c["coff"], rope_head_dim=ROPE, rotary_mode=c["rotary_mode"], cache_mode=c["cache_mode"], block_size=c["block_size"],
          table_dims=table.dim(), table_cols=table.shape[1] if table.dim() == 2 else 1, dtype=0 if c["dtype"] == torch.bfloat16 else 1,
          norm_eps=c["norm_eps"])
    for k, v in pointers.items():
        setattr(p, k, v)
    for k, v in over.items():
        setattr(p, k, v)
    return p
