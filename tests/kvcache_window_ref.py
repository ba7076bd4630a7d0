"""A float64 restatement of ``ffpa_attn_with_kvcache_window``'s visibility rule, written from the contract in its docstring and from nothing in the kernels.
The page gather, the capacity and the allowance are tests/kvcache_ref.py's.  Plain torch (any device): importable and testable without a GPU
(tests/test_kvcache_window.py)."""

from __future__ import annotations

import torch

import kvcache_ref as R


def effective_window(window, causal: bool) -> tuple:
  """``(left, right)`` as the call applies it: ``causal`` means right = 0, whatever ``right`` was given."""
  left, right = int(window[0]), int(window[1])
  return left, (0 if causal else right)


def visible(sq: int, n: int, window, causal: bool = False, device="cpu") -> torch.Tensor:
  """bool ``[sq, n]``: query token i (position ``pos_i = i + n - sq``) sees key j iff ``(left < 0 or j >= pos_i - left) and (right < 0 or j <= pos_i + right)``."""
  left, right = effective_window(window, causal)
  pos = torch.arange(sq, device=device)[:, None] + (n - sq)
  j = torch.arange(n, device=device)[None, :]
  ok = torch.ones((sq, n), dtype=torch.bool, device=device)
  if left >= 0:
    ok &= j >= pos - left
  if right >= 0:
    ok &= j <= pos + right
  return ok


def attend(q, k_cache, v_cache, lens, table=None, window=(-1, -1), causal: bool = False, scale: "float | None" = None):
  """``kvcache_ref.attend`` under the window: float64 softmax attention of ``q [B, Sq, Hq, D]`` over the first ``clamp(len_b, 0, capacity)`` keys of every sequence,
  token i seeing what ``visible`` says; GQA; rows without a visible key O = 0, LSE = -inf.  -> ``(o, lse [B, Hq, Sq], pmax, p2sum)`` float64, as that function."""
  B, sq, hq, d = q.shape
  hkv = k_cache.size(2)
  group = hq // hkv
  cap = R.capacity_of(k_cache, table)
  scale = d ** -0.5 if scale is None else scale
  dev = q.device
  o = torch.zeros((B, sq, hq, d), dtype=torch.float64, device=dev)
  lse = torch.full((B, hq, sq), float("-inf"), dtype=torch.float64, device=dev)
  pmax = torch.zeros((B, hq, sq), dtype=torch.float64, device=dev)
  p2sum = torch.zeros((B, hq, sq), dtype=torch.float64, device=dev)
  for b in range(B):
    n = min(max(int(lens[b]), 0), cap)
    if n == 0 or sq == 0:
      continue
    kb, vb = R.gather(k_cache, v_cache, table, b, n)
    kb, vb = kb.double().transpose(0, 1), vb.double().transpose(0, 1)  # [Hkv, n, D]
    vb = torch.nan_to_num(vb, nan=0.0)  # (a hidden key's V may hold NaN in the tests: its weight is an exact 0 below)
    qb = q[b].double().transpose(0, 1).reshape(hkv, group * sq, d)      # rows (head in group, token)
    s = torch.matmul(qb, torch.nan_to_num(kb, nan=0.0).transpose(1, 2)) * scale
    seen = visible(sq, n, window, causal, dev).repeat(group, 1)          # [group x Sq, n]
    s = s.masked_fill(~seen[None], float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    live = torch.isfinite(m)
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(e))
    o[b] = torch.matmul(p, vb).reshape(hq, sq, d).transpose(0, 1)
    row_lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))
    lse[b] = row_lse.reshape(hq, sq)
    pmax[b] = p.amax(dim=-1).reshape(hq, sq)
    p2sum[b] = p.pow(2).sum(dim=-1).reshape(hq, sq)
  return o, lse, pmax, p2sum


def seen_tiles(sq: int, n: int, window, causal: bool, keys: int) -> set:
  """The KV tiles (of ``keys`` keys) that hold a key visible to SOME token of a sequence of ``sq`` tokens and ``n`` keys: every other tile lies wholly outside
  every row's window."""
  cols = visible(sq, n, window, causal).any(dim=0).nonzero().flatten().tolist()
  return {j // keys for j in cols}
