"""The float64 yardstick of the sparse (top-k indexed) MLA latent-cache call: ``kvcache_ref.attend`` on a CONTIGUOUS cache built per token from the pool rows
its index list names — nothing of the kernels.  Plain torch (any device): tested without a GPU against a naive per-token softmax
(tests/test_kvcache_mla_sparse.py) and used by the GPU suite (tests/test_kvcache_mla_sparse_gpu.py) through ``kvcache_ref.check``."""

import torch

import kvcache_ref as R


def pool_rows(pool, slots):
  """Rows ``slots`` (int64 ``[n]``) of a latent pool: the flat ``[num_rows, Hkv, D]``, or ``[num_pages, page_size, Hkv, D]`` where slot r is row
  ``r % page_size`` of page ``r // page_size``.  Indexes the view: any strides."""
  if pool.dim() == 3:
    return pool[slots]
  return pool[slots // pool.size(1), slots % pool.size(1)]


def gathered(pool, indices, lens):
  """``(cache [T, max(n, 1), Hkv, D], lens)``: token t's slab holds ``pool[indices[t, :n_t]]`` in order, n_t = clamp(lens[t], 0, topk) — zeros behind it."""
  T, topk = indices.shape
  ns = [min(max(int(n), 0), topk) for n in lens]
  cache = torch.zeros((T, max(ns + [1]),) + tuple(pool.shape[-2:]), dtype=pool.dtype, device=pool.device)
  for t, n in enumerate(ns):
    if n:
      cache[t, :n] = pool_rows(pool, indices[t, :n].to(torch.int64))
  return cache, ns


def reference(q, pool, indices, lens, scale, head_dim_v):
  """``q [T, Hq, D]`` -> ``attend``'s tuple for T sequences of ONE token over the gathered slabs, value columns ``[:head_dim_v]``:
  ``(o [T, 1, Hq, dv], lse [T, Hq, 1], pmax, p2sum)`` float64 — the shapes ``kvcache_ref.check`` takes with ``out[:, None]`` / ``lse.t()[:, :, None]``."""
  cache, ns = gathered(pool, indices, lens)
  o, lse, pmax, p2sum = R.attend(q[:, None], cache, cache, ns, None, False, scale)
  return o[..., :head_dim_v].contiguous(), lse, pmax, p2sum


def visible_values(pool, indices, lens, head_dim_v):
  """``(largest |v|, RMS of v)`` over the rows the tokens attend to: what ``kvcache_ref.allowance`` wants of V when the rest of the pool holds NaN."""
  cache, ns = gathered(pool, indices, lens)
  return R.visible_values(cache[..., :head_dim_v], ns, None)
