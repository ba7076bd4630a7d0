"""A float64 restatement of ``ffpa_attn_varlen_with_kvcache`` — a RAGGED step over the KV cache: token rows packed by ``cu_seqlens_q``, the per-token append
with its two rotary position rules, attention per sequence — written from the contract in ffpa_attn_amd/kvcache.py's docstring.  Every sequence goes through the
uniform references (kvcache_ref.append / rotate, kvcache_softcap_ref.attend, which is kvcache_window_ref's under a cap of 0) as a batch of one; nothing of the
kernels is restated here.  Plus the builder of the ragged cases the tests share.  Plain torch: importable and testable without a GPU."""

from __future__ import annotations

import torch

import kvcache_ref as R
import kvcache_softcap_ref as S


def bounds(cu) -> list:
  """``cu_seqlens_q`` -> ``[(first row, end row), ...]`` per sequence."""
  cu = [int(x) for x in cu]
  return list(zip(cu[:-1], cu[1:]))


def _one(k_cache, v_cache, table, b: int):
  """The caches and the table as sequence b alone sees them: its slab (a view: writes land in the cache), or the whole pool with its row of the table."""
  if table is None:
    return k_cache[b:b + 1], v_cache[b:b + 1], None
  return k_cache, v_cache, table[b:b + 1]


def append(k_cache, v_cache, k, v, cu, lens, table=None, cos=None, sin=None, interleaved: bool = True, causal: bool = False, q=None, positions=None):
  """The append of the ragged call, IN PLACE on ``k_cache`` / ``v_cache``: key i of sequence b (row ``cu[b] + i`` of ``k`` / ``v [T, Hkv, D]``) at cache position
  ``max(len_b, 0) + i``, dropped at or past the capacity.  Rotary position without ``positions``: kvcache_ref.append's (key at its cache position, query token i
  at the same under ``causal``, at ``max(len_b, 0)`` otherwise); with ``positions [T]``: key AND query token of row t at ``positions[t]`` clamped to
  ``[0, seqlen_ro - 1]`` — the key still written at its slot.  Rows at or past ``cu[B]`` (padding) append nothing; their q rows come back unrotated.
  -> ``(q_rot float64 [T, Hq, D] | None, post-append lengths (list), rotated [(slab or page, row), ...])`` as kvcache_ref.append."""
  lens = [int(x) for x in lens]
  cap = R.capacity_of(k_cache, table)
  page = k_cache.size(1)
  used, rotated = [], []
  q_rot = q.double().clone() if (cos is not None and q is not None) else None
  for b, (s, e) in enumerate(bounds(cu)):
    kc, vc, tb = _one(k_cache, v_cache, table, b)
    qb = q[s:e][None] if q is not None else None
    if positions is None or cos is None:
      qr, u, rows = R.append(kc, vc, k[s:e][None], v[s:e][None], [lens[b]], tb, cos, sin, interleaved, causal, q=qb)
      rotated += [(slab if table is not None else b, row) for slab, row in rows]
    else:
      pos = torch.as_tensor(positions[s:e], dtype=torch.int64).clamp(min=0)
      kb = R.rotate(k[s:e], cos, sin, pos, interleaved).to(k_cache.dtype) if e > s else k[s:e]
      _, u, _ = R.append(kc, vc, kb[None], v[s:e][None], [lens[b]], tb)  # (already rotated: a plain write at the slots)
      for i in range(e - s):
        p = max(lens[b], 0) + i
        if p < cap:
          rotated.append((b, p) if table is None else (min(max(int(table[b, p // page]), 0), k_cache.size(0) - 1), p % page))
      qr = R.rotate(q[s:e], cos, sin, pos, interleaved)[None] if (q is not None and e > s) else None
    used.append(u[0])
    if q_rot is not None and qr is not None and e > s:
      q_rot[s:e] = qr[0]
  return q_rot, used, rotated


def attend(q, k_cache, v_cache, cu, lens, table=None, window=(-1, -1), causal: bool = False, scale: "float | None" = None, softcap: float = 0.0):
  """Float64 attention of the packed ``q [T, Hq, D]``: sequence b's rows ``cu[b] ... cu[b + 1]`` over its first ``clamp(len_b, 0, capacity)`` keys, bottom-right
  aligned, under ``window`` / ``causal`` / ``softcap`` (kvcache_softcap_ref.attend per sequence).  -> ``(o [1, N, Hq, D], lse [1, Hq, N], pmax, p2sum)`` float64
  over the ``N = cu[B]`` real rows — the batch-of-one shapes ``kvcache_ref.check`` takes (hand it ``out[None, :N]`` and ``lse[None, :, :N]``)."""
  parts = []
  for b, (s, e) in enumerate(bounds(cu)):
    kc, vc, tb = _one(k_cache, v_cache, table, b)
    parts.append(S.attend(q[s:e][None], kc, vc, [int(lens[b])], tb, window, causal, scale, softcap))
  return (torch.cat([p[0] for p in parts], dim=1),) + tuple(torch.cat([p[i] for p in parts], dim=2) for i in (1, 2, 3))


def effective_lens(seqs, lens, cap: int, appended: bool) -> list:
  """Keys every sequence attends over: ``min(max(len, 0) + Sq_b, cap)`` after an append, else ``clamp(len, 0, cap)``."""
  return [min(max(int(n), 0) + (int(s) if appended else 0), cap) for s, n in zip(seqs, lens)]


def tree_depths(seqs) -> list:
  """Depths of a small draft tree per sequence, token by token: node i hangs under node ``(i - 1) // 2`` (a binary heap: depths 0, 1, 1, 2, 2, 2, 2, 3 ...)."""
  out = []
  for n in seqs:
    out += [(i + 1).bit_length() - 1 for i in range(int(n))]
  return out


def make_case(seqs, lens, *, D: int = 512, heads=(8, 2), dtype="bf16", page: int = 64, seed: int = 0, rotary_dim: int = 0, pad: int = 0, pages_per_seq=None,
              capacity=None, bad_unused_ids: bool = False) -> dict:
  """A ragged step on the CPU: ``seqs`` query tokens per sequence against caches that hold ``max(lens[b], 0)`` keys (random data; every other row of the pool or
  slab is NaN), ``pad`` more token rows behind ``cu[B]`` (finite data: they must not be written anywhere).  ``page`` 0 = a contiguous cache of ``capacity`` keys;
  else shuffled pages, ``pages_per_seq`` per sequence, 3 pages nobody owns, and — ``bad_unused_ids`` — ids far outside the pool in the table entries past a
  sequence's last page after the append.  -> dict of tensors ``q k v cu lens table k_cache v_cache cos sin`` + ``seqs``, ``capacity``, ``dtype`` (name)."""
  g = torch.Generator().manual_seed(seed)
  dt = R.TORCH_DTYPE[dtype]
  hq, hkv = heads
  B, T = len(seqs), sum(seqs) + pad
  rnd = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float32).to(dt)
  q, k, v = rnd(T, hq, D), rnd(T, hkv, D), rnd(T, hkv, D)
  cu = torch.tensor([0] + [sum(seqs[:i + 1]) for i in range(B)], dtype=torch.int32)
  reach = max(max(n, 0) + s for n, s in zip(lens, seqs))
  table = None
  if page:
    pps = pages_per_seq or -(-reach // page) + 1
    cap = pps * page
    n_pages = B * pps + 3
    table = torch.randperm(n_pages, generator=g)[:B * pps].to(torch.int32).view(B, pps)
    kc, vc = torch.full((n_pages, page, hkv, D), float("nan"), dtype=dt), torch.full((n_pages, page, hkv, D), float("nan"), dtype=dt)
  else:
    cap = capacity or reach + 7
    kc, vc = torch.full((B, cap, hkv, D), float("nan"), dtype=dt), torch.full((B, cap, hkv, D), float("nan"), dtype=dt)
  for b in range(B):
    n = min(max(lens[b], 0), cap)
    if n:
      j = torch.arange(n)
      rows = (table[b].long()[j // page], j % page) if page else (torch.full((n,), b), j)
      kc[rows], vc[rows] = rnd(n, hkv, D), rnd(n, hkv, D)
  if page and bad_unused_ids:
    for b in range(B):
      first_unused = -(-min(max(lens[b], 0) + seqs[b], cap) // page)
      for j in range(first_unused, pps):
        table[b, j] = (-1, n_pages, 2 ** 31 - 1, -(2 ** 31))[(b + j) % 4]
  cos = sin = None
  if rotary_dim:
    ang = torch.rand((cap + 5, rotary_dim // 2), generator=g, dtype=torch.float64) * 6.283185307179586
    cos, sin = torch.cos(ang).to(dt), torch.sin(ang).to(dt)
  return dict(q=q, k=k, v=v, cu=cu, lens=torch.tensor(lens, dtype=torch.int32), table=table, k_cache=kc, v_cache=vc, cos=cos, sin=sin, seqs=list(seqs),
              capacity=cap, dtype=dtype)


def reference(t: dict, *, append_kv: bool = True, rotary: bool = True, interleaved: bool = True, causal: bool = False, window=(-1, -1), softcap: float = 0.0,
              positions=None, scale=None):
  """The float64 result of the call on clones of a case's caches -> ``(attend's tuple over the real rows, k_cache, v_cache after the append, rotated rows,
  effective lengths)``; the rotated copy of q that attends is rounded once to q's dtype, as in kvcache_ref.reference."""
  kc, vc = t["k_cache"].clone(), t["v_cache"].clone()
  q, lens, rotated = t["q"], [int(x) for x in t["lens"]], []
  cos, sin = (t["cos"], t["sin"]) if rotary else (None, None)
  if append_kv:
    q_rot, lens, rotated = append(kc, vc, t["k"], t["v"], t["cu"], lens, t["table"], cos, sin, interleaved, causal, q=q, positions=positions)
    if q_rot is not None:
      q = q_rot.to(t["q"].dtype)
  else:
    lens = effective_lens(t["seqs"], lens, t["capacity"], False)
  return attend(q, kc, vc, t["cu"], lens, t["table"], window, causal, scale, softcap), kc, vc, rotated, lens
