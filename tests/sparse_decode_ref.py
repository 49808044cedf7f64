"""Float64 restatement of block-sparse GQA decode attention (flash_decode_bnsd_with_gqa_share_sparse): plain loops over (sequence,
q head, list slot).  Test infrastructure, like mx_ref.py: the CPU test checks it against stored outputs of the reference kernel, the GPU
tests check the HIP kernel against it.

Per (b, h), kh = h // G, seq_len = min(seq_lens[b], max_kv_len): every slot t with lb = topk_idx[kh, b, t] >= 0 names a page
(block_table[b, lb], or req_to_token[req_pool_indices[b], min(lb * block_size, cols - 1)] // block_size, clamped to [0, num_pages - 1] when
sanitize_page_ids); its keys n with lb * block_size + n < seq_len take part with logit (q . k) * sm_scale.  A slot whose block starts at
or behind seq_len contributes nothing and its table entry is not read.  Duplicates count twice.  The sink adds one logit
(q . sink[h]) * sm_scale to the maximum and the denominator and has no value row.  A row without a key is zeros."""
import numpy as np
import torch


def _f64(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def _int(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().to(torch.int64).numpy()
    return np.asarray(t).astype(np.int64)


def _round_to(x, dtype):
    """float64 array rounded to a torch dtype (round-to-nearest-even through float32: exact for the exp() values in [0, 1] used here
    up to a double rounding far below the tolerances), back in float64."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(dtype).double().numpy()


def sparse_decode_ref(q, k_cache, v_cache, topk_idx, seq_lens, block_size, block_table=None, req_to_token=None, req_pool_indices=None,
                      max_num_blocks=None, num_pages=None, sanitize_page_ids=False, sink=None, sm_scale=None, round_p=None):
    """-> float64 [B, Hq, D].  round_p = a torch dtype: the softmax numerators are rounded to it before P.V (the denominator keeps the
    unrounded sum), which is what the kernels do with the cache dtype; None = exact."""
    q, k, v, sink = _f64(q), _f64(k_cache), _f64(v_cache), _f64(sink)
    idx, lens = _int(topk_idx), _int(seq_lens)
    bt, rtt, rpi = _int(block_table), _int(req_to_token), _int(req_pool_indices)
    assert (bt is None) != (rtt is None) and (rtt is None) == (rpi is None)
    B, Hq, D = q.shape
    bs, Hkv = k.shape[1], k.shape[2]
    assert bs == block_size and Hq % Hkv == 0
    G = Hq // Hkv
    if idx.shape[0] == Hq and Hq != Hkv:
        idx = idx[::G]                                        # per-q-head lists: the list of each group's first head
    assert idx.shape[0] == Hkv and idx.shape[1] == B
    if sm_scale is None:
        sm_scale = D ** -0.5
    max_kv_len = (bt.shape[1] if bt is not None else int(max_num_blocks)) * bs
    out = np.zeros((B, Hq, D), dtype=np.float64)
    for b in range(B):
        seq_len = min(int(lens[b]), max_kv_len)
        for kh in range(Hkv):
            keys, vals = [], []
            for t in range(idx.shape[2]):
                lb = int(idx[kh, b, t])
                if lb < 0 or lb * bs >= seq_len:
                    continue
                if bt is not None:
                    page = int(bt[b, lb])
                else:
                    page = int(rtt[int(rpi[b]), min(lb * bs, rtt.shape[1] - 1)]) // bs
                    if sanitize_page_ids:
                        page = min(max(page, 0), int(num_pages) - 1)
                n = min(bs, seq_len - lb * bs)
                keys.append(k[page, :n, kh])
                vals.append(v[page, :n, kh])
            if not keys:
                continue                                      # zeros, with or without a sink
            K, V = np.concatenate(keys), np.concatenate(vals)
            for h in range(kh * G, (kh + 1) * G):
                logits = (K @ q[b, h]) * sm_scale
                m = logits.max()
                extra = 0.0
                if sink is not None:
                    ls = float(q[b, h] @ sink[h]) * sm_scale
                    m = max(m, ls)
                    extra = np.exp(ls - m)
                p = np.exp(logits - m)
                denom = p.sum() + extra
                if round_p is not None:
                    p = _round_to(p, round_p)
                out[b, h] = (p @ V) / denom
    return out
