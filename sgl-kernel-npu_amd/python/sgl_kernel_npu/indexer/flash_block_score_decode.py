"""Block-score indexer of the block-sparse decode (reference: python/sgl_kernel_npu/sgl_kernel_npu/indexer/flash_block_score_decode.py).

`flash_decode_bnsd_with_topk_idx` scores every KV block of every sequence against the decode query (the block's largest logit, or its
log-sum-exp, in the log2 domain), forces the first `init_blocks` and the last `local_blocks` blocks in, and returns the `topk` best blocks
per query head: the `topk_idx` that `attention.gqa_share_sparse_attention.flash_decode_bnsd_with_gqa_share_sparse` attends to.  Score and
selection are two HIP launches (csrc/kernels/gqa_block_score.hip) sized from shapes and `max_seqlen` only, so the op can be captured in a
graph.  Two deliberate differences from the reference's Triton code, both in DESIGN.md: slots behind a row's last block hold -1 (the
reference repeats a candidate there, which the sparse decode would attend twice), and `topk` need not be a power of two (the reference's
per-chunk top-k keeps each chunk's FIRST topk blocks then).  Order: descending score, ties by ascending block id.

The full form (`disable_index_value=False`) also returns the dense attention output; it is served by composition -- this indexer plus the
sparse decode over the list of all blocks -- at the price of a second pass over K."""
from __future__ import annotations

from typing import Optional

import torch

import sgl_kernel_npu  # noqa: F401

MAX_SEQBLOCK = 16384      # the select kernel keeps one row of scores in 64 KB of LDS
MAX_TOPK = 1024


def _floor_power_of_2(x: int) -> int:
    x = int(x)
    return 1 if x < 2 else 1 << (x.bit_length() - 1)


def _is_power_of_two(n: int) -> bool:
    return n >= 1 and (n & (n - 1)) == 0


def _nominal_score_chunks(max_seqblock: int, blocks_per_chunk: int, max_chunks: int, batch_size: int, num_kv_heads: int) -> int:
    """The chunk count the reference's score launch would use (a power of two): only the `runtime_score_short_*` checks look at it; the
    HIP launch is not cut in such chunks."""
    if max_seqblock <= 0:
        return 1
    per = max(1, int(blocks_per_chunk))
    n = min(-(-max_seqblock // per), max(1, int(max_chunks)), max(1, 32768 // max(1, batch_size * max(1, num_kv_heads))))
    return _floor_power_of_2(max(1, n))


def _normalize_topk_idx_for_gqa(topk_idx: torch.Tensor, num_q_heads: int, num_kv_heads: int, gqa_group_size: int) -> torch.Tensor:
    """[num_kv_heads, B, topk] as it is; [num_q_heads, B, topk] reduced to the list of each group's first query head."""
    heads = topk_idx.shape[0]
    if heads == num_kv_heads:
        return topk_idx.contiguous()
    if heads != num_q_heads:
        raise AssertionError(f"topk_idx holds {heads} lists per sequence: neither num_kv_heads = {num_kv_heads} nor num_q_heads = {num_q_heads}")
    return topk_idx[::gqa_group_size].contiguous()


@torch.no_grad()
def append_local_block_to_topk_idx(topk_idx: torch.Tensor, seq_lens: torch.Tensor, block_size: int, num_blocks: int) -> torch.Tensor:
    """[H, B, topk] int32 -> [H, B, topk + 1]: entries outside [0, num_blocks) or that start behind the last key become -1 (order kept);
    slot topk holds the block of the last key, min(max(len - 1, 0) // block_size, num_blocks - 1), or -1 when it is among the entries."""
    assert topk_idx.ndim == 3
    assert topk_idx.dtype == torch.int32
    assert topk_idx.is_contiguous()
    assert seq_lens.ndim == 1
    assert seq_lens.shape[0] == topk_idx.shape[1]
    assert seq_lens.is_contiguous()
    assert block_size > 0
    assert num_blocks > 0
    return torch.ops.npu.topk_append_local_block(topk_idx, seq_lens, int(block_size), int(num_blocks))


@torch.no_grad()
def flash_decode_bnsd_with_topk_idx(
    q: torch.Tensor,  # [batch_size, num_q_heads, head_dim]
    sink: Optional[torch.Tensor],  # optional [num_q_heads, head_dim]
    k_cache_bnsd: torch.Tensor,  # [num_blocks, block_size, num_kv_heads, head_dim]
    v_cache_bnsd: Optional[torch.Tensor],
    block_table: Optional[torch.Tensor],  # [batch_size, max_num_blocks]
    seq_lens: torch.Tensor,  # [batch_size], or [batch_size * group] with packed_seq_lens
    max_seqlen: int,
    block_size: int,
    topk: int,
    init_blocks: int,
    local_blocks: int,
    sm_scale: Optional[float] = None,
    score_type: str = "max",
    disable_index_value: bool = False,
    num_kv_chunks: Optional[int] = None,
    max_num_kv_chunks: int = 8,
    use_triton_topk: Optional[bool] = None,
    num_topk_chunks: Optional[int] = None,
    use_chunked_score: bool = True,
    score_blocks_per_chunk: int = 16,
    score_max_chunks: int = 32,
    req_to_token: Optional[torch.Tensor] = None,
    req_pool_indices: Optional[torch.Tensor] = None,
    max_num_blocks: Optional[int] = None,
    num_pages: Optional[int] = None,
    sanitize_page_ids: bool = False,
    packed_seq_lens: bool = False,
    runtime_fill_only: bool = False,
    runtime_score_short_max_blocks: int = 0,
    runtime_score_short_chunks: int = 0,
    fused_append_local: bool = False,
    use_native: bool = True,
) -> tuple[Optional[torch.Tensor], torch.Tensor]:
    """Returns (o, topk_idx): topk_idx [num_q_heads, batch_size, topk] int32 ([.., topk + 1] with fused_append_local); o is None in the
    score-only form and the dense attention output [batch_size, num_q_heads, head_dim] otherwise.

    `num_kv_chunks`, `max_num_kv_chunks`, `use_triton_topk`, `num_topk_chunks`, `use_chunked_score`, `score_blocks_per_chunk`,
    `score_max_chunks`, `runtime_fill_only`, `runtime_score_short_*` and `use_native` are the reference's Ascend tuning knobs: accepted,
    checked where the reference checks them, and without effect on the result."""
    assert score_type in ("max", "lse")
    assert q.dtype in (torch.float16, torch.bfloat16)
    assert k_cache_bnsd.dtype == q.dtype
    assert seq_lens.dtype in (torch.int32, torch.int64)

    use_direct_page_lookup = req_to_token is not None
    assert (req_pool_indices is not None) == use_direct_page_lookup
    if use_direct_page_lookup:
        assert block_table is None
        assert disable_index_value
        assert req_to_token.ndim == 2
        assert req_to_token.dtype in (torch.int32, torch.int64)
        assert req_pool_indices.ndim == 1
        assert req_pool_indices.dtype in (torch.int32, torch.int64)
        assert max_num_blocks is not None and max_num_blocks > 0
        assert num_pages is not None and num_pages > 0
    else:
        assert block_table is not None
        assert block_table.dtype in (torch.int32, torch.int64)

    if not disable_index_value:
        assert v_cache_bnsd is not None
        assert v_cache_bnsd.dtype == q.dtype
        assert v_cache_bnsd.shape == k_cache_bnsd.shape

    batch_size, num_q_heads, head_dim = q.shape
    _, block_size_from_cache, num_kv_heads, cache_head_dim = k_cache_bnsd.shape
    assert block_size_from_cache == block_size
    assert cache_head_dim == head_dim
    assert num_q_heads % num_kv_heads == 0
    gqa_group_size = num_q_heads // num_kv_heads
    if packed_seq_lens:
        assert disable_index_value, "packed_seq_lens is score-only"
        assert seq_lens.shape[0] == batch_size * gqa_group_size
    else:
        assert seq_lens.shape[0] == batch_size
    if use_direct_page_lookup:
        assert req_pool_indices.shape[0] == batch_size
        assert max_num_blocks * block_size <= req_to_token.shape[1]
    else:
        assert block_table.shape[0] == batch_size

    if sm_scale is None:
        sm_scale = head_dim ** -0.5
    max_seqblock = (int(max_seqlen) + block_size - 1) // block_size

    def indexer():
        if topk <= 0:
            return torch.empty((num_q_heads, batch_size, 0), dtype=torch.int32, device=q.device)
        if fused_append_local:
            assert max_num_blocks is not None and max_num_blocks > 0
        assert 0 < max_seqblock <= MAX_SEQBLOCK, f"max_seqlen spans {max_seqblock} blocks; 1 .. {MAX_SEQBLOCK} are served"
        assert topk <= MAX_TOPK, f"topk = {topk}; up to {MAX_TOPK} are served"
        return torch.ops.npu.gqa_block_score_topk(
            q, k_cache_bnsd, block_table, seq_lens, int(max_seqlen), int(topk), int(init_blocks), int(local_blocks), float(sm_scale),
            score_type == "lse", req_to_token, req_pool_indices, int(max_num_blocks) if max_num_blocks else 0,
            int(num_pages) if use_direct_page_lookup else 0, bool(sanitize_page_ids), bool(packed_seq_lens), bool(fused_append_local))

    if disable_index_value:
        if topk > 0:
            chunks = _nominal_score_chunks(max_seqblock, score_blocks_per_chunk, score_max_chunks, batch_size, num_kv_heads)
            if runtime_score_short_chunks:
                runtime_score_short_chunks = min(runtime_score_short_chunks, chunks)
            if runtime_score_short_max_blocks or runtime_score_short_chunks:
                assert runtime_score_short_max_blocks > 0
                assert runtime_score_short_chunks > 0
                assert runtime_score_short_chunks <= chunks
                assert _is_power_of_two(runtime_score_short_chunks)
        return None, indexer()

    if num_kv_chunks is not None:
        num_kv_chunks = int(num_kv_chunks)
        assert num_kv_chunks >= 1
        assert _is_power_of_two(num_kv_chunks)
    topk_idx = indexer()
    # dense attention = the sparse decode over the list of all blocks, built on the device (blocks at or behind a sequence's end are
    # dropped by that kernel); enough chunks that none holds more than its 1024 list slots
    n_list = max(1, min(max_seqblock, block_table.shape[1]))
    every = torch.arange(n_list, dtype=torch.int32, device=q.device).expand(num_kv_heads, batch_size, n_list)
    chunks = int(torch.ops.npu.gqa_share_sparse_num_chunks(batch_size, num_kv_heads, n_list))
    while chunks * 1024 < n_list:
        chunks *= 2
    lens = seq_lens.clamp(max=n_list * block_size)
    o = torch.ops.npu.gqa_share_sparse_decode(q, sink, k_cache_bnsd, v_cache_bnsd, block_table, lens, every, float(sm_scale), chunks)
    return o, topk_idx
