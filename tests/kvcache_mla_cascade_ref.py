"""The plan of ffpa_attn_with_kvcache_mla_cascade restated in plain torch (any device), from the formulas in its docstring and in include/ffpa_attn.h and from
nothing in the kernel: the effective prefix of every group, the packed queries' boundaries by group, the prefix rows and the shifted suffix rows.  Importable and
testable without a GPU (tests/test_kvcache_mla_cascade.py); the GPU tests hold the plan kernel to it exactly."""

from __future__ import annotations

import torch


def plan(lens, block_table, cu_group_seqs, shared_prefix_len, page_size: int, seqlen_q: int, causal: bool, capacity: int):
  """``lens [B]`` (the keys every sequence holds after the step's append, not clamped), ``block_table [B, W]``, ``cu_group_seqs [G + 1] | None`` (one group),
  ``shared_prefix_len``: an int or ``[G]`` -> ``(cu_q_prefix [G + 1], prefix_lens [G], prefix_table [G, W], suffix_table [B, W], suffix_lens [B])``, int32::

      P_g = page_size * floor(clamp(min(shared_prefix_len[g], min over b in g of (clamp(len_b, 0, capacity) - (Sq - 1 if causal else 0))), 0, capacity) / page_size)

  (an empty group: 0); ``prefix_table[g]`` is the row of the group's first sequence (an empty group: row ``min(start, B - 1)`` — the contract allows any in-range
  row); ``suffix_table[b, j] = block_table[b, min(j + P_g / page_size, W - 1)]``; ``suffix_lens[b] = clamp(len_b, 0, capacity) - P_g``."""
  B, W = block_table.shape
  dev = block_table.device
  cu = [0, B] if cu_group_seqs is None else [int(x) for x in cu_group_seqs.tolist()]
  G = len(cu) - 1
  stated = [int(shared_prefix_len)] * G if isinstance(shared_prefix_len, int) else [int(x) for x in shared_prefix_len.tolist()]
  held = [min(max(int(x), 0), capacity) for x in lens.tolist()]
  back = seqlen_q - 1 if causal else 0
  prefix = []
  for g in range(G):
    members = held[cu[g]:cu[g + 1]]
    if not members:
      prefix.append(0)
      continue
    p = min(stated[g], min(n - back for n in members))
    prefix.append(min(max(p, 0), capacity) // page_size * page_size)
  i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
  table = block_table.to(torch.int64)
  prefix_table = torch.stack([table[min(cu[g], B - 1)] for g in range(G)]).to(torch.int32)
  suffix_table = torch.empty((B, W), dtype=torch.int32, device=dev)
  suffix_lens = [0] * B
  cols = torch.arange(W, device=dev)
  for g in range(G):
    for b in range(cu[g], cu[g + 1]):
      suffix_table[b] = table[b][(cols + prefix[g] // page_size).clamp(max=W - 1)].to(torch.int32)
      suffix_lens[b] = held[b] - prefix[g]
  return i32([c * seqlen_q for c in cu]), i32(prefix), prefix_table, suffix_table, i32(suffix_lens)
