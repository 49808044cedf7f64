"""Block-sparse GQA decode attention over precomputed top-k KV blocks (reference:
python/sgl_kernel_npu/sgl_kernel_npu/attention/gqa_share_sparse_attention.py:635-878).

The decode half of the block-sparse attention whose prefill half is `flash_prefill_bnsd_blockq_sparse_fia`: every sequence attends to the
KV blocks its list names (logical block ids, -1 = none, anywhere in the list), per KV head, with an optional vector sink per q head.
One HIP launch (csrc/kernels/gqa_sparse_decode.hip) per chunk count of 1, plus a merge launch for more; the chunk count is chosen from
shapes only, so the op can be captured in a graph.  The indexer that produces `topk_idx` is `indexer.flash_block_score_decode.flash_decode_bnsd_with_topk_idx`.  No reference test
exists for this file (parity is pinned by outputs of the reference kernel stored under tests/golden/)."""
from __future__ import annotations

from typing import Optional

import torch

import sgl_kernel_npu  # noqa: F401


def _is_power_of_two(n: int) -> bool:
    return n >= 1 and (n & (n - 1)) == 0


@torch.no_grad()
def flash_decode_bnsd_with_gqa_share_sparse(
    q: torch.Tensor,  # [batch_size, num_q_heads, head_dim]
    sink: Optional[torch.Tensor],  # optional [num_q_heads, head_dim]
    k_cache_bnsd: torch.Tensor,  # [num_blocks, block_size, num_kv_heads, head_dim]
    v_cache_bnsd: torch.Tensor,  # same shape
    block_table: Optional[torch.Tensor],  # [batch_size, max_num_blocks]
    seq_lens: torch.Tensor,  # [batch_size]
    block_size: int,
    topk_idx: torch.Tensor,  # [num_kv_heads or num_q_heads, batch_size, topk]
    sm_scale: Optional[float] = None,
    num_topk_chunks: Optional[int] = None,
    max_num_topk_chunks: int = 8,
    req_to_token: Optional[torch.Tensor] = None,
    req_pool_indices: Optional[torch.Tensor] = None,
    max_num_blocks: Optional[int] = None,
    num_pages: Optional[int] = None,
    sanitize_page_ids: bool = False,
    topk_blocks_per_step: int = 1,
    prefetch_idx: bool = False,
    num_warps: Optional[int] = None,
    num_stages: Optional[int] = None,
    use_native: bool = True,
) -> torch.Tensor:
    """Sparse decode attention using BNSD KV cache and precomputed topk blocks.  Returns [batch_size, num_q_heads, head_dim].

    `topk_blocks_per_step`, `prefetch_idx`, `num_warps`, `num_stages` and `use_native` are the reference's Ascend tuning knobs: accepted,
    checked where the reference checks them, and without effect on the result."""
    assert q.dtype in (torch.float16, torch.bfloat16)
    assert k_cache_bnsd.dtype == q.dtype
    assert v_cache_bnsd.dtype == q.dtype
    assert k_cache_bnsd.shape == v_cache_bnsd.shape

    use_direct_page_lookup = req_to_token is not None
    assert (req_pool_indices is not None) == use_direct_page_lookup
    if use_direct_page_lookup:
        assert block_table is None
        assert req_to_token.ndim == 2
        assert req_to_token.dtype in (torch.int32, torch.int64)
        assert req_pool_indices.ndim == 1
        assert req_pool_indices.dtype in (torch.int32, torch.int64)
        assert max_num_blocks is not None and max_num_blocks > 0
        assert num_pages is not None and num_pages > 0
    else:
        assert block_table is not None
        assert block_table.dtype in (torch.int32, torch.int64)

    batch_size, num_q_heads, head_dim = q.shape
    _, block_size_from_cache, num_kv_heads, cache_head_dim = k_cache_bnsd.shape
    assert block_size_from_cache == block_size
    assert cache_head_dim == head_dim
    assert num_q_heads % num_kv_heads == 0
    assert seq_lens.shape[0] == batch_size
    assert topk_idx.shape[1] == batch_size
    assert topk_idx.shape[0] in (num_kv_heads, num_q_heads)
    if use_direct_page_lookup:
        assert req_pool_indices.shape[0] == batch_size
        assert max_num_blocks * block_size <= req_to_token.shape[1]
    else:
        assert block_table.shape[0] == batch_size

    max_topk = topk_idx.shape[2]
    if sm_scale is None:
        sm_scale = head_dim ** -0.5

    if num_topk_chunks is None:
        # the library's choice (shapes and the CU count), bounded by the caller's limit; a power of two either way
        num_topk_chunks = torch.ops.npu.gqa_share_sparse_num_chunks(batch_size, num_kv_heads, max_topk)
        while num_topk_chunks > max(1, int(max_num_topk_chunks)):
            num_topk_chunks //= 2
    else:
        num_topk_chunks = int(num_topk_chunks)
    assert num_topk_chunks >= 1
    assert _is_power_of_two(num_topk_chunks)
    assert num_topk_chunks <= max(1, max_topk)
    assert _is_power_of_two(max(1, int(topk_blocks_per_step)))

    return torch.ops.npu.gqa_share_sparse_decode(
        q, sink, k_cache_bnsd, v_cache_bnsd, block_table, seq_lens, topk_idx, float(sm_scale), num_topk_chunks, req_to_token,
        req_pool_indices, int(max_num_blocks) if use_direct_page_lookup else 0, int(num_pages) if use_direct_page_lookup else 0,
        bool(sanitize_page_ids))
