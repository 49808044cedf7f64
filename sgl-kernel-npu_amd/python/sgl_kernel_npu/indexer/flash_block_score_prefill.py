"""Block-score indexer of the block-sparse prefill (reference: python/sgl_kernel_npu/sgl_kernel_npu/indexer/flash_block_score_prefill.py).

`flash_prefill_bnsd_with_topk_idx` scores every query token of a varlen prefill chunk against every KV block it can see (the block's
largest logit, or its log-sum-exp, in the log2 domain) and returns the `topk` best blocks per (index head, token): with
`per_query_seq_lens` and one index head per kv head that is the `topk_idx [H, total_q, topk + 1]` -- causal-local block appended -- which
`attention.fia_blockq_attention.flash_prefill_bnsd_blockq_sparse_fia` attends to.  Score and selection are one HIP launch each
(csrc/kernels/gqa_block_score_prefill.hip), sized from shapes and `max_seqlen` only.

Three deliberate differences from the reference's Triton code, all in DESIGN.md §4.3.3:
  * the causal mask compares the key position with the token's TRUE position `seq_lens[r] - q_len[r] + i`; the reference compares with the
    packed token index, which hides a cached prefix and leaks future keys into every request after the first (the two agree for one request
    without a prefix; `torch.ops.npu.gqa_prefill_block_score(..., query_pos=...)` takes any convention);
  * in the non-fused selection, slots behind a row's visible blocks hold -1 (the reference's `torch.topk` over -inf names arbitrary blocks);
  * `block_size_q`, `num_score_chunks` and `qblock_mappings` are the reference's tiling and precomputation: accepted, checked, without effect.

One extension: `max_seqlen`.  When given, nothing is read back from the device (the reference's `seq_lens.max().item()` is skipped) and the
call can be captured in a graph.

The forms that also return `idx_o`, the dense causal attention of the index heads, are served by composition: the score op plus the paged
GQA decode kernel with one query row per token.  Price: a `[total_q, max_blocks]` int32 table built on the device and K / V re-read for
every token (through L2); a tiled prefill attention kernel is not part of this module."""
from __future__ import annotations

from typing import Optional

import torch

import sgl_kernel_npu  # noqa: F401

MAX_SEQBLOCK = 16384
MAX_TOPK = 1024
_INDEX = (torch.int32, torch.int64)


def _max_seqblock(seq_lens: torch.Tensor, block_size_k: int, max_seqlen: Optional[int]) -> tuple[int, int]:
    if max_seqlen is None:
        max_seqlen = int(seq_lens.max().item()) if seq_lens.numel() else 0
    max_seqlen = int(max_seqlen)
    blocks = (max_seqlen + block_size_k - 1) // block_size_k
    assert blocks <= MAX_SEQBLOCK, f"max_seqlen spans {blocks} blocks; up to {MAX_SEQBLOCK} are served"
    return max_seqlen, blocks


def _check_score_args(q, k_cache_bnsd, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size_q, block_size_k, sm_scale, score_type):
    assert score_type in ("max", "lse")
    assert q.ndim == 3 and k_cache_bnsd.ndim == 4
    assert q.dtype in (torch.float16, torch.bfloat16)
    assert k_cache_bnsd.dtype == q.dtype
    assert q.shape[1] % k_cache_bnsd.shape[2] == 0
    assert k_cache_bnsd.shape[1] == block_size_k, "block_size_k is the page size of the cache"
    assert k_cache_bnsd.shape[3] == q.shape[2]
    assert block_size_q > 0
    assert sm_scale > 0
    assert cu_seqlens.ndim == 1 and cu_seqlens.dtype in _INDEX
    assert seq_lens.ndim == 1 and seq_lens.dtype in _INDEX
    assert cu_seqlens.shape[0] == seq_lens.shape[0] + 1
    assert req_to_token.ndim == 2 and req_to_token.dtype in _INDEX
    assert req_pool_indices.ndim == 1 and req_pool_indices.dtype in _INDEX
    assert req_pool_indices.shape[0] == seq_lens.shape[0]


@torch.no_grad()
def flash_prefill_bnsd_score(
    q: torch.Tensor,  # [total_q, num_idx_heads, head_dim]
    k_cache_bnsd: torch.Tensor,  # [num_pages, page_size, num_kv_heads, head_dim]
    cu_seqlens: torch.Tensor,  # [bs+1]
    seq_lens: torch.Tensor,  # [bs] total KV len
    req_to_token: torch.Tensor,
    req_pool_indices: torch.Tensor,
    block_size_q: int,
    block_size_k: int,  # == page_size
    sm_scale: float,
    score_type: str = "max",
    num_score_chunks: Optional[int] = None,
    qblock_mappings: Optional[tuple] = None,
    max_seqlen: Optional[int] = None,
) -> torch.Tensor:
    """-> score [num_idx_heads, total_q, max_seqblock_k] fp32, -inf where token and block share no visible key; every element is written."""
    _check_score_args(q, k_cache_bnsd, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size_q, block_size_k, sm_scale, score_type)
    max_seqlen, max_seqblock_k = _max_seqblock(seq_lens, block_size_k, max_seqlen)
    total_q, num_idx_heads, _ = q.shape
    if total_q == 0 or max_seqblock_k == 0:
        return torch.empty((num_idx_heads, total_q, max_seqblock_k), device=q.device, dtype=torch.float32)
    return torch.ops.npu.gqa_prefill_block_score(q, k_cache_bnsd, cu_seqlens.contiguous(), seq_lens.contiguous(), req_to_token,
                                                 req_pool_indices.contiguous(), max_seqlen, float(sm_scale), score_type == "lse", None)


@torch.no_grad()
def flash_prefill_bnsd_topk_from_score(
    score: torch.Tensor,  # [num_kv_heads, total_q, max_seqblock_k] fp32
    per_query_seq_lens: torch.Tensor,  # [total_q] int32 -- per-query causal KV len
    topk: int,
    block_size_k: int,
) -> torch.Tensor:
    """Fused top-k + causal-local-block append -> topk_idx [num_kv_heads, total_q, topk + 1] int32: per row the topk best scores above
    -inf in descending order (ties: the lowest block id), of which those with block * block_size_k > len - 1 become -1 in place, then -1;
    slot topk holds min(max(len - 1, 0) // block_size_k, max_seqblock_k - 1), or -1 when that block is among the entries."""
    num_kv_heads, total_q, max_seqblock_k = score.shape
    assert score.dtype == torch.float32, "score must be fp32"
    assert per_query_seq_lens.dtype == torch.int32
    assert per_query_seq_lens.shape[0] == total_q
    if topk <= 0 or total_q == 0:
        return torch.empty((num_kv_heads, total_q, topk + 1 if topk > 0 else 0), dtype=torch.int32, device=score.device)
    assert topk <= MAX_TOPK, f"topk = {topk}; up to {MAX_TOPK} are served"
    assert 0 < max_seqblock_k <= MAX_SEQBLOCK
    return torch.ops.npu.prefill_topk_from_score(score, per_query_seq_lens.contiguous(), int(topk), int(block_size_k), True)


def _select(score: torch.Tensor, q: torch.Tensor, k_cache_bnsd: torch.Tensor, per_query_seq_lens, topk: int, block_size_k: int) -> torch.Tensor:
    if per_query_seq_lens is not None and q.shape[1] == k_cache_bnsd.shape[2]:
        return flash_prefill_bnsd_topk_from_score(score, per_query_seq_lens, topk, block_size_k)
    if topk <= 0 or score.shape[1] == 0:
        return torch.empty((score.shape[0], score.shape[1], max(topk, 0)), dtype=torch.int32, device=score.device)
    assert topk <= MAX_TOPK, f"topk = {topk}; up to {MAX_TOPK} are served"
    if score.shape[2] == 0:
        return torch.full((score.shape[0], score.shape[1], topk), -1, dtype=torch.int32, device=score.device)
    return torch.ops.npu.prefill_topk_from_score(score, None, int(topk), int(block_size_k), False)


@torch.no_grad()
def flash_prefill_bnsd_score_attn(
    q: torch.Tensor,  # [total_q, num_idx_heads, head_dim]  (index Q)
    k_cache_bnsd: torch.Tensor,  # [num_pages, page_size, num_kv_heads, head_dim]
    v_cache_bnsd: torch.Tensor,  # [num_pages, page_size, num_kv_heads, head_dim]
    cu_seqlens: torch.Tensor,
    seq_lens: torch.Tensor,
    req_to_token: torch.Tensor,
    req_pool_indices: torch.Tensor,
    block_size_q: int,
    block_size_k: int,
    sm_scale: float,
    score_type: str = "max",
    qblock_mappings: Optional[tuple] = None,
    max_seqlen: Optional[int] = None,
):
    """-> (score, idx_o): the block scores and the dense causal attention of the index heads [total_q, num_idx_heads, head_dim] (zeros for
    tokens no request owns).  idx_o is served by composition: a [total_q, max_blocks] int32 block table gathered from `req_to_token` on the
    device and the paged GQA decode kernel with one query row per token (kv length = position + 1), so K and V are re-read for every token."""
    assert v_cache_bnsd.dtype == q.dtype
    assert v_cache_bnsd.shape == k_cache_bnsd.shape
    max_seqlen, max_seqblock_k = _max_seqblock(seq_lens, block_size_k, max_seqlen)
    score = flash_prefill_bnsd_score(q, k_cache_bnsd, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size_q, block_size_k, sm_scale,
                                     score_type, qblock_mappings=qblock_mappings, max_seqlen=max_seqlen)
    total_q, n = q.shape[0], seq_lens.shape[0]
    idx_o = torch.zeros_like(q)
    if total_q == 0 or n == 0 or max_seqblock_k == 0:
        return score, idx_o
    dev = q.device
    cu = cu_seqlens.to(torch.int64)
    lens = seq_lens.to(torch.int64).clamp(min=0, max=max_seqblock_k * block_size_k)
    q_lens = (cu[1:] - cu[:-1]).clamp(min=0)
    counts = torch.cat([q_lens, (total_q - cu[-1:]).clamp(min=0)])      # the tokens behind cu[n] count as one more request
    owner = torch.repeat_interleave(torch.arange(n + 1, device=dev), counts, output_size=total_q)
    owned = owner < n
    owner = owner.clamp(max=n - 1)
    pos = seq_lens.to(torch.int64)[owner] - q_lens[owner] + (torch.arange(total_q, device=dev) - cu[:-1][owner])
    kv_lens = torch.minimum(lens[owner], pos + 1)
    owned &= kv_lens > 0
    cols = (torch.arange(max_seqblock_k, device=dev) * block_size_k).clamp(max=req_to_token.shape[1] - 1)
    table = (req_to_token[req_pool_indices.to(torch.int64)[owner][:, None], cols[None, :]] // block_size_k).to(torch.int32)
    out = torch.empty_like(idx_o)
    torch.ops.npu.decode_gqa(q, k_cache_bnsd, v_cache_bnsd, out, kv_lens.clamp(min=1).to(torch.int32), float(sm_scale), int(block_size_k), table, 0)
    return score, torch.where(owned[:, None, None], out, idx_o)


@torch.no_grad()
def flash_prefill_bnsd_indexer(
    q: torch.Tensor,  # idx_q [total_q, num_idx_heads, idx_dim]
    k_cache_bnsd: torch.Tensor,  # idx_k
    v_cache_bnsd: torch.Tensor,  # idx_v
    cu_seqlens: torch.Tensor,
    seq_lens: torch.Tensor,
    req_to_token: torch.Tensor,
    req_pool_indices: torch.Tensor,
    block_size_q: int,
    block_size_k: int,
    topk: int,
    sm_scale: float,
    score_type: str = "max",
    qblock_mappings: Optional[tuple] = None,
    per_query_seq_lens: Optional[torch.Tensor] = None,
    max_seqlen: Optional[int] = None,
):
    """-> (idx_o, topk_idx): `flash_prefill_bnsd_score_attn` (composition, see there) and the selection of
    `flash_prefill_bnsd_with_topk_idx`."""
    score, idx_o = flash_prefill_bnsd_score_attn(q, k_cache_bnsd, v_cache_bnsd, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size_q,
                                                 block_size_k, sm_scale, score_type, qblock_mappings, max_seqlen=max_seqlen)
    return idx_o, _select(score, q, k_cache_bnsd, per_query_seq_lens, topk, block_size_k)


@torch.no_grad()
def flash_prefill_bnsd_with_topk_idx(
    q: torch.Tensor,  # idx_q [total_q, num_idx_heads, idx_dim]
    k_cache_bnsd: torch.Tensor,  # idx_k [num_pages, page_size, num_kv_heads, idx_dim]
    cu_seqlens: torch.Tensor,
    seq_lens: torch.Tensor,
    req_to_token: torch.Tensor,
    req_pool_indices: torch.Tensor,
    block_size_q: int,
    block_size_k: int,
    topk: int,
    sm_scale: float,
    score_type: str = "max",
    qblock_mappings: Optional[tuple] = None,
    per_query_seq_lens: Optional[torch.Tensor] = None,
    max_seqlen: Optional[int] = None,
) -> torch.Tensor:
    """With `per_query_seq_lens` and num_idx_heads == num_kv_heads: topk_idx [H, total_q, topk + 1] (flash_prefill_bnsd_topk_from_score).
    Otherwise [num_idx_heads, total_q, topk]: the min(topk, visible blocks) best blocks, descending score, ties by ascending id, then -1.
    topk <= 0: an empty [num_idx_heads, total_q, 0] without a launch."""
    if topk <= 0:
        _check_score_args(q, k_cache_bnsd, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size_q, block_size_k, sm_scale, score_type)
        return torch.empty((q.shape[1], q.shape[0], 0), dtype=torch.int32, device=q.device)
    score = flash_prefill_bnsd_score(q, k_cache_bnsd, cu_seqlens, seq_lens, req_to_token, req_pool_indices, block_size_q, block_size_k, sm_scale,
                                     score_type, qblock_mappings=qblock_mappings, max_seqlen=max_seqlen)
    return _select(score, q, k_cache_bnsd, per_query_seq_lens, topk, block_size_k)
