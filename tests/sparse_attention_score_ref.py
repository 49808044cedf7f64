"""Float64 restatement of torch.ops.npu.npu_sparse_attention_score (block-sparse GQA attention over per-token block lists): plain loops
over (token, kv head, slot, q head).  Test infrastructure, like sparse_decode_ref.py: the CPU test pins it to that restatement and to
hand-computed cases, the GPU tests check the HIP kernel against it.

Token t is token j of the request b whose running sum of actual_seq_lengths (lengths, not cumulative; None = one token per request) covers
it; pos = actual_seq_lengths_kv[b] - actual_seq_lengths[b] + j.  Of select_idx[kh, t, :] the first n slots are live (n = topK, or
select_num_idx[kh, t] clamped to [0, topK]); slots behind n are not looked at.  A live slot with id lb contributes all block_size keys of page
block_table[b, lb] if lb < pos // block_size and the first pos % block_size + 1 if lb == pos // block_size; it is dropped -- its table entry
not read -- when lb < 0, lb > pos // block_size or lb >= columns.  Duplicates count twice.  out = softmax((q . k) * scale) . v, no sink;
zeros for a token without a contributing key, with pos < 0, or behind the sum of the lengths.

FP8: the inputs are taken as float8.double() * scale: q by q_dequant_scale[b, h, pos // block_size], a block's k / v rows by
k_dequant_scale[b, kh, lb] / v_dequant_scale[b, kh, lb]."""
import numpy as np
import torch

from sparse_decode_ref import _f64, _int, _round_to


def sparse_attention_score_ref(query, key, value, select_idx, block_table, select_num_idx=None, q_dequant_scale=None, k_dequant_scale=None,
                               v_dequant_scale=None, actual_seq_lengths=None, actual_seq_lengths_kv=None, scale_value=0.0, round_p=None,
                               fold_sv=None):
    """-> float64 [T, Hq, D].  round_p = a torch dtype: the softmax numerators are rounded to it before P.V (the denominator keeps the
    unrounded sum), as the kernel does with its engine dtype; fold_sv = a torch dtype: the dequantised value rows v8 * sv are rounded to it,
    as the kernel does when it folds the v scale into the rows it stages (fp16); None = exact."""
    q, k, v = _f64(query), _f64(key), _f64(value)
    idx, bt, num = _int(select_idx), _int(block_table), _int(select_num_idx)
    qlen, kvlen = _int(actual_seq_lengths), _int(actual_seq_lengths_kv)
    sq, sk, sv = _f64(q_dequant_scale), _f64(k_dequant_scale), _f64(v_dequant_scale)
    assert kvlen is not None
    T, Hq, D = q.shape
    bs = k.shape[1]
    Hkv, Q, topk = idx.shape
    batch, columns = bt.shape
    assert Hq % Hkv == 0 and Q >= T and k.shape == v.shape and k.shape[2] == Hkv
    G = Hq // Hkv
    scale = D ** -0.5 if abs(scale_value) <= 1e-9 else float(scale_value)
    if qlen is None:
        assert T == batch
        qlen = np.ones(batch, dtype=np.int64)
    out = np.zeros((T, Hq, D), dtype=np.float64)
    t = 0
    for b in range(batch):
        for j in range(max(int(qlen[b]), 0)):
            if t >= T:
                break
            pos = int(kvlen[b]) - int(qlen[b]) + j
            _one_token(out, t, b, pos, q, k, v, idx, bt, num, sq, sk, sv, bs, Hkv, G, topk, columns, scale, round_p, fold_sv)
            t += 1
    return out                                                # rows t .. T - 1 lie behind the sum of the lengths: zeros


def _one_token(out, t, b, pos, q, k, v, idx, bt, num, sq, sk, sv, bs, Hkv, G, topk, columns, scale, round_p, fold_sv):
    if pos < 0:
        return
    diag = pos // bs
    for kh in range(Hkv):
        n = topk if num is None else min(max(int(num[kh, t]), 0), topk)
        keys, vals = [], []
        for s in range(n):
            lb = int(idx[kh, t, s])
            if lb < 0 or lb > diag or lb >= columns:
                continue
            page = int(bt[b, lb])
            cnt = bs if lb < diag else pos % bs + 1
            kr, vr = k[page, :cnt, kh], v[page, :cnt, kh]
            if sk is not None:
                kr, vr = kr * sk[b, kh, lb], vr * sv[b, kh, lb]
                if fold_sv is not None:
                    vr = _round_to(vr, fold_sv)
            keys.append(kr)
            vals.append(vr)
        if not keys:
            continue
        K, V = np.concatenate(keys), np.concatenate(vals)
        for h in range(kh * G, (kh + 1) * G):
            qv = q[t, h] if sq is None else q[t, h] * sq[b, h, diag]
            logits = (K @ qv) * scale
            p = np.exp(logits - logits.max())
            denom = p.sum()
            if round_p is not None:
                p = _round_to(p, round_p)
            out[t, h] = (p @ V) / denom
