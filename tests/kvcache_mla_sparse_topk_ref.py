"""The definition of ``ffpa_mla_sparse_topk_slots`` / ``ffpa_mla_sparse_slots`` in plain torch (any device) — nothing of the kernel: the visible-length rule, a
stable descending sort of the first ``n`` scores, the first ``topk`` of it, an ascending sort, the block-table translation, the -1 tail.  Integer results: every
comparison against it is exact.  Tested without a GPU against brute force and against the two torch helpers (tests/test_kvcache_mla_sparse_topk.py), used by the
GPU suite (tests/test_kvcache_mla_sparse_topk_gpu.py)."""

import torch


def token_sequences(T, cache_seqlens, cu_seqlens_q):
  """Per row t: ``(b, i, S)`` — token i of the S query tokens of sequence b — or ``None`` for a padding row (at or past ``cu_seqlens_q[B]``)."""
  B = cache_seqlens.numel()
  if cu_seqlens_q is None:
    assert T % B == 0
    Sq = T // B
    return [(t // Sq, t % Sq, Sq) for t in range(T)]
  cu = [int(x) for x in cu_seqlens_q]
  rows = [None] * T
  for b in range(B):
    for t in range(cu[b], min(cu[b + 1], T)):
      rows[t] = (b, t - cu[b], cu[b + 1] - cu[b])
  return rows


def visible(L, S, i, N, causal):
  """How many leading columns token i of S sees of a sequence of length L: the bottom-right alignment of the ragged calls."""
  return min(max(L - (S - 1 - i) if causal else L, 0), N)


def select(rows, n, topk):
  """The selected positions of score rows that share one visible length (float32 ``[..., N]``) -> int64 ``[..., min(n, topk)]``, ascending: all of
  ``0 ... n - 1`` if ``n <= topk``, else the first ``topk`` of a stable descending sort of ``rows[..., :n]`` (NaN the largest, -0.0 == +0.0, the lower position
  first among equals)."""
  if n <= topk:
    return torch.arange(n, dtype=torch.int64, device=rows.device).expand(rows.shape[:-1] + (n,))
  order = torch.sort(rows[..., :n], dim=-1, descending=True, stable=True).indices
  return torch.sort(order[..., :topk], dim=-1).values


def translate(pos, table_row, page_size):
  """Positions (int64 ``[k]``, all >= 0) of one sequence -> int64 slots through its row of page ids (``None``: the positions themselves)."""
  if table_row is None:
    return pos
  page = table_row.to(torch.int64)[(pos // page_size).clamp(max=table_row.numel() - 1)]
  return page * page_size + pos % page_size


def _finish(rows, T, topk, device):
  indices = torch.full((T, topk), -1, dtype=torch.int32, device=device)
  lens = torch.zeros(T, dtype=torch.int32, device=device)
  for t, slots in enumerate(rows):
    if slots is not None:
      indices[t, :slots.numel()] = slots.to(torch.int32)  # (int64 -> int32 wraps, as the kernel's int32 store does)
      lens[t] = slots.numel()
  return indices, lens


def topk_slots(scores, topk, cache_seqlens, block_table=None, page_size=None, *, cu_seqlens_q=None, causal=True):
  """``ffpa_mla_sparse_topk_slots`` -> ``(indices int32 [T, topk], topk_lens int32 [T])``."""
  T, N = scores.shape
  lens = [int(x) for x in cache_seqlens]
  rows = []
  for t, where in enumerate(token_sequences(T, cache_seqlens, cu_seqlens_q)):
    if where is None:
      rows.append(None)
      continue
    b, i, S = where
    pos = select(scores[t], visible(lens[b], S, i, N, causal), topk)
    rows.append(translate(pos, None if block_table is None else block_table[b], page_size))
  return _finish(rows, T, topk, scores.device)


def slots(positions, cache_seqlens, block_table=None, page_size=None, *, cu_seqlens_q=None):
  """``ffpa_mla_sparse_slots`` -> ``(indices int32 [T, topk], topk_lens int32 [T])``: the entries >= 0 in their order, translated; -1 behind them."""
  T, topk = positions.shape
  rows = []
  for t, where in enumerate(token_sequences(T, cache_seqlens, cu_seqlens_q)):
    if where is None:
      rows.append(None)
      continue
    pos = positions[t][positions[t] >= 0].to(torch.int64)
    rows.append(translate(pos, None if block_table is None else block_table[where[0]], page_size))
  return _finish(rows, T, topk, positions.device)
