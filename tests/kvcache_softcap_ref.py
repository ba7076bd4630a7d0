"""A float64 restatement of ``ffpa_attn_with_kvcache_softcap``, written from the contract in its docstring and from nothing in the kernels: it is
``kvcache_window_ref.attend`` with the cap applied to the scaled scores BEFORE the visibility mask — ``score = c * tanh(scale * q.k / c)``, a hidden key has weight
0 —, and returns the same tuple.  The page gather and the capacity are tests/kvcache_ref.py's, the visibility rule tests/kvcache_window_ref.py's.  Plain torch (any
device): importable and testable without a GPU (tests/test_kvcache_softcap.py)."""

from __future__ import annotations

import torch

import kvcache_ref as R
import kvcache_window_ref as W


def cap_scores(s: torch.Tensor, softcap: float) -> torch.Tensor:
  """``softcap * tanh(s / softcap)`` on scaled scores; ``softcap == 0`` means "off"."""
  return s if softcap == 0 else softcap * torch.tanh(s / softcap)


def attend(q, k_cache, v_cache, lens, table=None, window=(-1, -1), causal: bool = False, scale: "float | None" = None, softcap: float = 0.0):
  """Float64 softmax attention of ``q [B, Sq, Hq, D]`` over the first ``clamp(len_b, 0, capacity)`` keys of every sequence with capped scores, token i seeing what
  ``kvcache_window_ref.visible`` says; GQA; rows without a visible key O = 0, LSE = -inf.  -> ``(o, lse [B, Hq, Sq], pmax, p2sum)`` float64."""
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
    s = cap_scores(torch.matmul(qb, torch.nan_to_num(kb, nan=0.0).transpose(1, 2)) * scale, softcap)  # the cap first ...
    seen = W.visible(sq, n, window, causal, dev).repeat(group, 1)        # [group x Sq, n]
    s = s.masked_fill(~seen[None], float("-inf"))                        # ... the mask on the capped score
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


def tanh_f32(y):
  """The kernel's tanh chain (csrc/ffpa_fwd_m16_kernel.h ``m16_softcap_tanh``) restated operation by operation in float32 numpy:
  ``e = exp2(y * 2 log2(e))``, ``t = fma(-2, 1 / (1 + e), 1)`` (the product by 2 is exact, so the fma is one rounding of ``1 - 2 r``)."""
  import numpy as np

  with np.errstate(over="ignore", under="ignore"):
    y = np.asarray(y, dtype=np.float32)
    e = np.exp2(y * np.float32(2.8853900817779268))
    r = np.float32(1.0) / (np.float32(1.0) + e)
    return (np.float32(1.0) - np.float32(2.0) * r).astype(np.float32)
