"""CPU-only: the float64 restatement of block-sparse GQA decode (tests/sparse_decode_ref.py) reproduces every stored output of the
reference Triton kernel (tests/golden/gqa_sparse_ref_fp16_*.npz, written by gen_sparse_decode_golden.py) within the fp16 criterion that
test_gqa_gpu.py applies to reference-kernel outputs: atol = 1e-3, rtol = 2**-10.  That pins the semantics the GPU tests hold the HIP
kernel to."""
import glob
import os

import numpy as np
import pytest
import torch

from sparse_decode_ref import sparse_decode_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = sorted(glob.glob(os.path.join(GOLD, "gqa_sparse_ref_fp16_*.npz")))


def ref_kwargs(z):
    """The restatement's keyword arguments for a stored case."""
    kw = dict(sink=z["sink"] if "sink" in z else None, sm_scale=float(z["sm_scale"]))
    if "block_table" in z:
        kw.update(block_table=z["block_table"])
    else:
        kw.update(req_to_token=z["req_to_token"], req_pool_indices=z["req_pool_indices"], max_num_blocks=int(z["max_num_blocks"]),
                  num_pages=int(z["num_pages"]), sanitize_page_ids=bool(z["sanitize_page_ids"]))
    return kw


def test_the_stored_cases_cover_what_they_must():
    assert len(PATHS) >= 4
    seen = set()
    for path in PATHS:
        assert os.path.getsize(path) < 500 * 1000, path
        z = np.load(path)
        Hq, Hkv, bs = z["q"].shape[1], z["k"].shape[2], int(z["block_size"])
        idx, lens = z["topk_idx"], z["seq_lens"]
        seen.add("hkv1" if Hkv == 1 else "hkv>1")
        seen.add("sink" if "sink" in z else "no sink")
        seen.add("direct" if "req_to_token" in z else "table")
        seen.add(f"block {bs}")
        if idx.shape[0] == Hq and Hq != Hkv:
            seen.add("per-q-head lists")
            idx = idx[::Hq // Hkv]
        for kh in range(idx.shape[0]):
            for b in range(idx.shape[1]):
                row = idx[kh, b]
                if (row < 0).all():
                    seen.add("all -1")
                real = np.nonzero(row >= 0)[0]
                if len(real) and (row[:real[-1]] < 0).any():
                    seen.add("holes")
                last = (int(lens[b]) - 1) // bs
                if len(real) and int(lens[b]) % bs and last in row[:real[-1]].tolist():
                    seen.add("partial block not last")
    assert seen >= {"hkv1", "hkv>1", "sink", "no sink", "direct", "table", "block 16", "block 64", "per-q-head lists", "all -1", "holes",
                    "partial block not last"}, seen


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p) for p in PATHS])
def test_restatement_reproduces_reference_kernel_outputs(path):
    z = np.load(path)
    got = sparse_decode_ref(z["q"], z["k"], z["v"], z["topk_idx"], z["seq_lens"], int(z["block_size"]), **ref_kwargs(z))
    want = z["out"].astype(np.float64)
    err = np.abs(got - want)
    print(os.path.basename(path), "max abs error", err.max())
    assert (err <= 1e-3 + 2.0 ** -10 * np.abs(want)).all(), err.max()


def test_a_row_without_a_valid_block_is_exactly_zero():
    hit = 0
    for path in PATHS:
        z = np.load(path)
        Hq, Hkv = z["q"].shape[1], z["k"].shape[2]
        G = Hq // Hkv
        idx = z["topk_idx"][::G] if z["topk_idx"].shape[0] == Hq and Hq != Hkv else z["topk_idx"]
        got = sparse_decode_ref(z["q"], z["k"], z["v"], z["topk_idx"], z["seq_lens"], int(z["block_size"]), **ref_kwargs(z))
        for kh in range(Hkv):
            for b in range(idx.shape[1]):
                if (idx[kh, b] < 0).all():
                    hit += 1
                    assert (z["out"][b, kh * G:(kh + 1) * G] == 0).all() and (got[b, kh * G:(kh + 1) * G] == 0).all()
    assert hit >= 1
    # and with a sink: the sink has no value row
    q = torch.randn(1, 4, 64).to(torch.float16)
    kv = torch.randn(3, 16, 1, 64).to(torch.float16)
    out = sparse_decode_ref(q, kv, kv, np.full((1, 1, 4), -1), [40], 16, block_table=np.zeros((1, 3), dtype=np.int32), sink=torch.randn(4, 64))
    assert (out == 0).all()
