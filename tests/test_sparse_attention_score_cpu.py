"""CPU-only: pins the float64 restatement of npu_sparse_attention_score (tests/sparse_attention_score_ref.py) to what the project already
trusts -- the restatement of block-sparse decode (tests/sparse_decode_ref.py, itself pinned to stored reference-kernel outputs) -- and to
hand-computed tiny cases for what that one does not have: the live prefix, the per-token causal end, padding tokens, pos < 0, FP8 scales."""
import glob
import os

import numpy as np
import pytest
import torch

from sparse_attention_score_ref import sparse_attention_score_ref
from sparse_decode_ref import sparse_decode_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = sorted(glob.glob(os.path.join(GOLD, "gqa_sparse_ref_fp16_*.npz")))


@pytest.mark.parametrize("seed", range(8))
def test_one_token_per_request_equals_the_decode_restatement(seed):
    """No select_num_idx, no sink, a block table: the op is flash_decode_bnsd_with_gqa_share_sparse.  Lists hold -1 anywhere, duplicates,
    blocks at or behind the sequence's end and behind the table's extent; lengths reach 0, 1, a block boundary and above the table."""
    rng = np.random.default_rng(seed)
    B, Hkv, G, D, bs, topk = 4, 2, int(rng.integers(1, 4)), 16, int(rng.choice([4, 8])), 7
    columns = 6
    pages = B * columns
    q = rng.standard_normal((B, Hkv * G, D))
    k, v = rng.standard_normal((pages, bs, Hkv, D)), rng.standard_normal((pages, bs, Hkv, D))
    bt = rng.permutation(pages).reshape(B, columns)
    lens = np.array([int(rng.integers(0, columns * bs + 9)), 1, 3 * bs, columns * bs + 5])
    idx = rng.integers(-1, columns + 2, size=(Hkv, B, topk))
    idx[:, :, 3] = idx[:, :, 1]                               # duplicates
    idx[0, 2] = -1
    got = sparse_attention_score_ref(q, k, v, idx, bt, actual_seq_lengths_kv=lens, scale_value=0.3)
    want = sparse_decode_ref(q, k, v, idx, lens, bs, block_table=bt, sm_scale=0.3)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(want).max() > 0 and (got[2, :G] == 0).all()
    ones = sparse_attention_score_ref(q, k, v, idx, bt, actual_seq_lengths=np.ones(B, dtype=np.int32), actual_seq_lengths_kv=lens, scale_value=0.3)
    assert np.array_equal(ones, got)
    # rounding P is the same switch in both
    got16 = sparse_attention_score_ref(q, k, v, idx, bt, actual_seq_lengths_kv=lens, scale_value=0.3, round_p=torch.float16)
    want16 = sparse_decode_ref(q, k, v, idx, lens, bs, block_table=bt, sm_scale=0.3, round_p=torch.float16)
    assert np.abs(got16 - want16).max() <= 1e-12


def test_stored_reference_kernel_outputs_with_a_table_and_no_sink():
    """Every stored gqa_sparse_ref_fp16_*.npz case that uses a block table and no sink must be reproduced at the criterion of
    test_gqa_sparse_decode_cpu.py (atol = 1e-3, rtol = 2**-10).  Of the four stored cases today, a and c carry a sink and b and d use the
    request map, so none qualifies: the loop is empty and the pin is test_one_token_per_request_equals_the_decode_restatement, whose other
    side reproduces all four stored cases."""
    for path in PATHS:
        z = np.load(path)
        if "sink" in z or "block_table" not in z:
            continue
        Hq, Hkv = z["q"].shape[1], z["k"].shape[2]
        idx = z["topk_idx"][::Hq // Hkv] if z["topk_idx"].shape[0] == Hq and Hq != Hkv else z["topk_idx"]
        got = sparse_attention_score_ref(z["q"], z["k"], z["v"], idx, z["block_table"], actual_seq_lengths_kv=z["seq_lens"],
                                         scale_value=float(z["sm_scale"]))
        want = z["out"].astype(np.float64)
        assert (np.abs(got - want) <= 1e-3 + 2.0 ** -10 * np.abs(want)).all(), path


def softmax_av(qv, K, V, scale):
    w = np.exp((K @ qv) * scale)
    return (w / w.sum()) @ V


def tiny(seed=0, T=6, Hq=2, Hkv=1, D=4, bs=4, pages=5, columns=3, batch=3, topk=3):
    rng = np.random.default_rng(seed)
    return dict(q=rng.standard_normal((T, Hq, D)), k=rng.standard_normal((pages, bs, Hkv, D)), v=rng.standard_normal((pages, bs, Hkv, D)),
                bt=np.array([[4, 0, 2], [1, 3, 0], [2, 2, 2]][:batch])[:, :columns])


def test_per_token_causal_end_and_padding_by_hand():
    """Requests of 3, 0 and 2 query tokens, kv lengths 6, 9, 1 (the third request's first token stands at position -1), one padding token."""
    c = tiny()
    q, k, v, bt = c["q"], c["k"], c["v"], c["bt"]
    idx = np.array([[[0, 1, 2], [1, 0, -1], [1, 1, 0], [0, 0, 0], [0, 1, 2], [0, 1, 2]]])
    out = sparse_attention_score_ref(q, k, v, idx, bt, actual_seq_lengths=[3, 0, 2], actual_seq_lengths_kv=[6, 9, 1], scale_value=0.5)
    # token 0: request 0, pos 3: the diagonal block is 0 (all 4 keys of page 4); blocks 1 and 2 lie behind it
    for h in range(2):
        assert np.allclose(out[0, h], softmax_av(q[0, h], k[4, :, 0], v[4, :, 0], 0.5), atol=1e-14)
    # token 1: pos 4: block 1 is the diagonal one with 1 key (page 0), block 0 whole; list order (1, 0)
    K = np.concatenate([k[0, :1, 0], k[4, :, 0]])
    V = np.concatenate([v[0, :1, 0], v[4, :, 0]])
    assert np.allclose(out[1, 1], softmax_av(q[1, 1], K, V, 0.5), atol=1e-14)
    # token 2: pos 5: block 1 twice (2 keys each time) and block 0
    K = np.concatenate([k[0, :2, 0], k[0, :2, 0], k[4, :, 0]])
    V = np.concatenate([v[0, :2, 0], v[0, :2, 0], v[4, :, 0]])
    assert np.allclose(out[2, 0], softmax_av(q[2, 0], K, V, 0.5), atol=1e-14)
    # token 3: request 2 (request 1 has no token), pos 1 - 2 + 0 = -1: zeros; token 4: pos 0: one key of page 2 -> its value row
    assert (out[3] == 0).all()
    assert np.allclose(out[4, 0], v[2, 0, 0], atol=1e-14) and np.allclose(out[4, 1], v[2, 0, 0], atol=1e-14)
    # token 5 lies behind the sum of the lengths
    assert (out[5] == 0).all()


def test_live_prefix_by_hand():
    c = tiny(seed=1)
    q, k, v, bt = c["q"], c["k"], c["v"], c["bt"]
    kvlen = [12, 12, 12]
    clean = np.array([[[0, 2, -1], [1, -1, -1], [-1, -1, -1], [2, 0, 1], [0, 1, 2], [-1, 1, -1]]])
    dirty = clean.copy()
    num = np.array([[2, 1, 0, 3, 5, 2]])                      # 5 clamps to topK; 0 and "only -1 live" give zeros rows
    for t in range(6):
        dirty[0, t, min(int(num[0, t]), 3):] = 10 ** 6        # would leave the table if looked at
    kw = dict(actual_seq_lengths=[2, 2, 2], actual_seq_lengths_kv=kvlen, scale_value=0.0)
    got = sparse_attention_score_ref(q, k, v, dirty, bt, select_num_idx=num, **kw)
    want = sparse_attention_score_ref(q, k, v, np.where(dirty == 10 ** 6, -1, dirty), bt, **kw)
    assert np.array_equal(got, want)
    assert (got[2] == 0).all() and (got[0] != 0).all()
    # token 1 (request 0, pos 11, diagonal block 2): its one live slot is block 1, whole; scale_value 0 means 1 / sqrt(D)
    assert np.allclose(got[1, 0], softmax_av(q[1, 0], k[0, :, 0], v[0, :, 0], 0.5), atol=1e-14)
    # a negative count is 0
    neg = sparse_attention_score_ref(q, k, v, dirty, bt, select_num_idx=np.full((1, 6), -3), **kw)
    assert (neg == 0).all()


def test_a_count_below_topk_cuts_off_valid_blocks_by_hand():
    """Every slot holds a block that would contribute: only the count keeps the slots behind it out."""
    c = tiny(seed=3)
    q, k, v, bt = c["q"], c["k"], c["v"], c["bt"]
    kw = dict(actual_seq_lengths=[1, 1, 0], actual_seq_lengths_kv=[10, 7, 0], scale_value=0.5)
    idx = np.array([[[0, 2, 1], [1, 0, 0]] + [[0, 0, 0]] * 4])
    num = np.array([[1, 2, 3, 3, 3, 3]])
    out = sparse_attention_score_ref(q, k, v, idx, bt, select_num_idx=num, **kw)
    # token 0: request 0, pos 9 (diagonal block 2, 2 keys): of (0, 2, 1) only block 0 (page 4, whole) is live
    assert np.allclose(out[0, 0], softmax_av(q[0, 0], k[4, :, 0], v[4, :, 0], 0.5), atol=1e-14)
    # token 1: request 1, pos 6 (diagonal block 1, 3 keys of page 3): of (1, 0, 0) the diagonal block and block 0 (page 1) once
    K = np.concatenate([k[3, :3, 0], k[1, :, 0]])
    V = np.concatenate([v[3, :3, 0], v[1, :, 0]])
    assert np.allclose(out[1, 1], softmax_av(q[1, 1], K, V, 0.5), atol=1e-14)
    # with the count one higher the next slot joins: the diagonal block (2 keys of page 2) for token 0, block 0 a second time for token 1
    out = sparse_attention_score_ref(q, k, v, idx, bt, select_num_idx=num + 1, **kw)
    K = np.concatenate([k[4, :, 0], k[2, :2, 0]])
    V = np.concatenate([v[4, :, 0], v[2, :2, 0]])
    assert np.allclose(out[0, 0], softmax_av(q[0, 0], K, V, 0.5), atol=1e-14)
    K = np.concatenate([k[3, :3, 0], k[1, :, 0], k[1, :, 0]])
    V = np.concatenate([v[3, :3, 0], v[1, :, 0], v[1, :, 0]])
    assert np.allclose(out[1, 1], softmax_av(q[1, 1], K, V, 0.5), atol=1e-14)
    # and it equals the list cut to -1 behind the count, and differs from the whole list
    cut = np.array([[[0, -1, -1], [1, 0, -1]] + [[0, 0, 0]] * 4])
    assert np.array_equal(sparse_attention_score_ref(q, k, v, idx, bt, select_num_idx=num, **kw), sparse_attention_score_ref(q, k, v, cut, bt, **kw))
    assert np.abs(sparse_attention_score_ref(q, k, v, idx, bt, **kw) - sparse_attention_score_ref(q, k, v, cut, bt, **kw))[:2].max() > 1e-3


def test_fp8_scales_by_hand():
    """Scales are indexed [b, h, pos // bs] (q) and [b, kh, lb] (k, v); fold_sv rounds the dequantised value rows."""
    rng = np.random.default_rng(2)
    T, Hq, D, bs = 2, 2, 8, 4
    q8 = torch.from_numpy(rng.standard_normal((T, Hq, D))).to(torch.float8_e4m3fn)
    k8 = torch.from_numpy(rng.standard_normal((3, bs, 1, D))).to(torch.float8_e4m3fn)
    v8 = torch.from_numpy(rng.standard_normal((3, bs, 1, D))).to(torch.float8_e4m3fn)
    bt = np.array([[2, 0], [1, 2]])
    sq = rng.uniform(0.5, 2.0, (2, Hq, 2))
    sk, sv = rng.uniform(0.5, 2.0, (2, 1, 2)), rng.uniform(0.5, 2.0, (2, 1, 2)) / 3
    idx = np.array([[[1, 0], [0, 1]]])
    out = sparse_attention_score_ref(q8, k8, v8, idx, bt, q_dequant_scale=sq, k_dequant_scale=sk, v_dequant_scale=sv,
                                     actual_seq_lengths_kv=[6, 3], scale_value=0.25)
    qd, kd, vd = q8.double().numpy(), k8.double().numpy(), v8.double().numpy()
    # token 0: request 0, pos 5, diagonal block 1 (2 keys of page 0) then block 0 (page 2); q scale column 1
    K = np.concatenate([kd[0, :2, 0] * sk[0, 0, 1], kd[2, :, 0] * sk[0, 0, 0]])
    V = np.concatenate([vd[0, :2, 0] * sv[0, 0, 1], vd[2, :, 0] * sv[0, 0, 0]])
    assert np.allclose(out[0, 1], softmax_av(qd[0, 1] * sq[0, 1, 1], K, V, 0.25), atol=1e-13)
    # token 1: request 1, pos 2: block 0 (page 1) with 3 keys, q scale column 0; block 1 lies behind the causal end
    assert np.allclose(out[1, 0], softmax_av(qd[1, 0] * sq[1, 0, 0], kd[1, :3, 0] * sk[1, 0, 0], vd[1, :3, 0] * sv[1, 0, 0], 0.25), atol=1e-13)
    folded = sparse_attention_score_ref(q8, k8, v8, idx, bt, q_dequant_scale=sq, k_dequant_scale=sk, v_dequant_scale=sv,
                                        actual_seq_lengths_kv=[6, 3], scale_value=0.25, fold_sv=torch.float16)
    assert 0 < np.abs(folded - out).max() < 2.0 ** -10 * np.abs(vd).max() * sv.max()


def test_the_op_is_registered_with_the_reference_schema():
    """What SGLang probes for: torch.ops.npu.npu_sparse_attention_score, argument for argument as the reference registers it."""
    import sgl_kernel_npu  # noqa: F401
    schema = str(torch.ops.npu.npu_sparse_attention_score.default._schema)
    assert schema == ("npu::npu_sparse_attention_score(Tensor query, Tensor key, Tensor value, Tensor select_idx, Tensor block_table, "
                      "Tensor? select_num_idx=None, Tensor? q_dequant_scale=None, Tensor? k_dequant_scale=None, Tensor? v_dequant_scale=None, "
                      "Tensor? actual_seq_lengths=None, Tensor? actual_seq_lengths_kv=None, int num_key_value_heads=1, float scale_value=1., "
                      "int block_size=128, int top_k=16, int inner_precise=0) -> Tensor"), schema
