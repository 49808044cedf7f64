"""The cooperative layout launch hands every workgroup's totals to the workgroups behind it inside the launch (write-through stores,
`sc1` loads, no fence around the arrival counter: csrc/ep/layout_dev.h).  A hand-off of that kind fails, when it fails, as a stale
word read under uneven load from a cache that still holds the previous call's bytes -- so: 40 calls back to back on ONE workspace and ONE
pair of sync words, a freshly drawn routing per call, a second stream copying 256 MB meanwhile, and every word of every output of
every call compared with the oracle."""
import functools

import numpy as np
import pytest
import torch

from oracle import ep as O

pytestmark = pytest.mark.gpu

CALLS = 40


@functools.lru_cache(maxsize=None)
def routings(T, K, E):
    """CALLS routings of T tokens: K distinct experts per token (a random start and a random stride coprime to E), ~10 % of the ids -1."""
    rng = np.random.default_rng(T * 131 + E)
    strides = np.array([b for b in range(1, E) if np.gcd(b, E) == 1], np.int64)
    out = []
    for _ in range(CALLS):
        a = rng.integers(0, E, (T, 1))
        b = strides[rng.integers(0, strides.size, (T, 1))]
        idx = (a + b * np.arange(K, dtype=np.int64)[None, :]) % E
        idx[rng.random((T, K)) < 0.1] = -1
        out.append(np.ascontiguousarray(idx))
    return out


@functools.lru_cache(maxsize=None)
def expected(T, K, E, W):
    want = [O.dispatch_layout(idx, E, W) for idx in routings(T, K, E)]
    for w in want:
        w["send_data_offset"] = O.send_data_offset(w["num_tokens_per_expert"])
    return want


KEYS = ("num_tokens_per_rank", "num_tokens_per_expert", "is_token_in_rank", "send_token_idx_small", "send_data_offset")


def run_calls(T, K, E, W, i32):
    import ep_harness as Hh
    from capi import ptr, stream_ptr
    lib = Hh.lib()
    dev = torch.device("cuda")
    want = expected(T, K, E, W)
    idxs = [torch.from_numpy(i).to(dev) for i in routings(T, K, E)]
    if i32:
        idxs = [t.int() for t in idxs]
    o32 = dict(dtype=torch.int32, device=dev)
    outs = [[torch.full(s, -3, **o32) for s in ((W,), (E,), (T, W), (T, K), (E,))] for _ in range(CALLS)]
    wsb = lib.mi_ep_dispatch_layout_workspace(T, K, E)
    ws = torch.full((wsb,), 0x5A, dtype=torch.uint8, device=dev)
    words = torch.zeros(2, **o32)
    status = torch.zeros(4, **o32)
    words_after = torch.full((CALLS, 2), -1, **o32)                    # the sync words as every call left them
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for c in range(CALLS):
        with torch.cuda.stream(side):
            dst.copy_(src, non_blocking=True)
        o = outs[c]
        Hh.ck(lib.mi_ep_dispatch_layout(ptr(idxs[c]), int(i32), T, K, E, W, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4]),
                                        ptr(ws), wsb, ptr(words), ptr(status), stream_ptr()))
        words_after[c].copy_(words, non_blocking=True)
    torch.cuda.synchronize()
    assert int(status[0]) == 0, status.tolist()
    assert not words_after.any(), words_after.tolist()
    for c in range(CALLS):
        for k, t in zip(KEYS, outs[c]):
            assert np.array_equal(t.cpu().numpy(), want[c][k]), (k, c)


# 257: two workgroups, a last unit of one token; 1025: one token past four workgroups; 4096: the benchmark's grid; 40000: the 64-token units
@pytest.mark.parametrize("T", [257, 1025, 4096, 40000])
@pytest.mark.parametrize("W", [1, 8])
@pytest.mark.parametrize("i32", [False, True], ids=["int64", "int32"])
def test_layout_handoff_back_to_back(T, W, i32):
    run_calls(T, 8, 256, W, i32)


@pytest.mark.parametrize("i32", [False, True], ids=["int64", "int32"])
def test_layout_handoff_padded_row(i32):
    """E + W = 28 words: the row is padded to one whole 128-byte line."""
    run_calls(1025, 8, 24, 4, i32)
