"""A float64 restatement of ``ffpa_attn_with_kvcache_tree`` (tree-mask attention over a KV cache: the verification step of tree speculative decoding), written
from the contract in ffpa_attn_amd/kvcache.py's docstring and from nothing in the kernels.  Built on ``kvcache_ref.gather`` and returning ``kvcache_ref.attend``'s
4-tuple, so ``kvcache_ref.check`` / ``kvcache_ref.allowance`` apply unchanged; plus the mask builders and the seeded case generator the tree tests share.
Plain torch (any device): importable and testable without a GPU (tests/test_tree_ref.py)."""

from __future__ import annotations

import random

import torch

import kvcache_ref as R


def visible(tree_mask, b: int, n: int, sq: int, device=None):
  """``[Sq, n]`` bool: which of the ``n`` keys of sequence ``b`` each of its ``sq`` draft tokens sees.  Key p < n - sq (the prefix): every token; key
  n - sq + j: token i iff ``tree_mask[b, i, j]`` (a ``[Sq, Sq]`` mask serves every sequence).  Draft positions below 0 (n < sq) do not exist."""
  m = tree_mask if tree_mask.dim() == 2 else tree_mask[b]
  dev = m.device if device is None else device
  p = torch.arange(n, device=dev)
  j = p - (n - sq)                                                   # draft index of key p (negative: the prefix)
  draft = m.to(dev)[:, j.clamp(min=0)]                               # [Sq, n]
  return torch.where((j < 0)[None, :], torch.ones_like(draft), draft)


def attend_tree(q, k_cache, v_cache, lens, table, tree_mask, scale: "float | None" = None):
  """Float64 softmax attention of ``q [B, Sq, Hq, D]`` over the first ``clamp(len_b, 0, capacity)`` keys of every sequence under a tree mask (``visible``):
  ``kvcache_ref.attend`` with the causal comparison replaced by the mask — the same operations in the same order, so ``tril(ones)`` reproduces
  ``attend(causal=True)`` and all ones ``attend(causal=False)`` to the bit.  GQA (query head h reads KV head h // group); rows without a visible key O = 0,
  LSE = -inf.  -> ``(o [B, Sq, Hq, D], lse [B, Hq, Sq], pmax [B, Hq, Sq], p2sum [B, Hq, Sq])`` float64."""
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
    kb, vb = kb.double().transpose(0, 1), vb.double().transpose(0, 1)         # [Hkv, n, D]
    qb = q[b].double().transpose(0, 1).reshape(hkv, group * sq, d)             # [Hkv, group x Sq, D], rows (head in group, token)
    s = torch.matmul(qb, kb.transpose(1, 2)) * scale                           # [Hkv, group x Sq, n]
    hidden = ~visible(tree_mask, b, n, sq, dev).repeat(group, 1)               # [group x Sq, n]
    s = s.masked_fill(hidden[None], float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    live = torch.isfinite(m)
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(e))
    ob = torch.matmul(p, vb)                                                   # [Hkv, group x Sq, D]
    o[b] = ob.reshape(hq, sq, d).transpose(0, 1)
    row_lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))
    lse[b] = row_lse.reshape(hq, sq)
    pmax[b] = p.amax(dim=-1).reshape(hq, sq)
    p2sum[b] = p.pow(2).sum(dim=-1).reshape(hq, sq)
  return o, lse, pmax, p2sum


def brute_force(q, k_cache, v_cache, lens, table, tree_mask, scale: "float | None" = None):
  """``(o, lse)`` of the same call one query row at a time, keys picked by a Python loop over the contract's two rules: what ``attend_tree`` must equal."""
  B, sq, hq, d = q.shape
  hkv = k_cache.size(2)
  group = hq // hkv
  cap = R.capacity_of(k_cache, table)
  scale = d ** -0.5 if scale is None else scale
  o = torch.zeros((B, sq, hq, d), dtype=torch.float64)
  lse = torch.full((B, hq, sq), float("-inf"), dtype=torch.float64)
  for b in range(B):
    n = min(max(int(lens[b]), 0), cap)
    if n == 0:
      continue
    kb, vb = R.gather(k_cache, v_cache, table, b, n)
    m = tree_mask if tree_mask.dim() == 2 else tree_mask[b]
    for i in range(sq):
      keys = [p for p in range(n) if p < n - sq or bool(m[i, p - (n - sq)])]
      if not keys:
        continue
      for h in range(hq):
        s = (kb[keys, h // group].double() @ q[b, i, h].double()) * scale
        w = torch.softmax(s, dim=0)
        o[b, i, h] = w @ vb[keys, h // group].double()
        lse[b, h, i] = torch.logsumexp(s, dim=0)
  return o, lse


# ----------------------------------------------------------------------------- masks
MASK_KINDS = ("tree", "random", "tril", "ones", "sparse")


def tree_mask_from_parents(parents) -> torch.Tensor:
  """``[Sq, Sq]`` bool of a draft tree: node i sees its ancestors and itself (``parents[i]`` < i, or -1 for a root)."""
  n = len(parents)
  m = torch.zeros((n, n), dtype=torch.bool)
  for i in range(n):
    j = i
    while j >= 0:
      m[i, j] = True
      j = parents[j]
  return m


def draw_mask(kind: str, sq: int, rng: random.Random) -> torch.Tensor:
  """One ``[Sq, Sq]`` mask: ``tree`` a random parent array; ``random`` arbitrary bits (a clear diagonal, later nodes, all-False rows); ``sparse`` mostly clear
  rows with a few bits anywhere — always the last column somewhere when there is one (bit Sq - 1: bit 63 at Sq = 64); ``tril`` / ``ones`` the two masks the
  plain call can express."""
  if kind == "tree":
    return tree_mask_from_parents([rng.randrange(-1, i) for i in range(sq)])
  if kind == "tril":
    return torch.tril(torch.ones((sq, sq), dtype=torch.bool))
  if kind == "ones":
    return torch.ones((sq, sq), dtype=torch.bool)
  density = 0.5 if kind == "random" else 0.12
  m = torch.tensor([[rng.random() < density for _ in range(sq)] for _ in range(sq)], dtype=torch.bool).reshape(sq, sq)
  if kind == "random" and sq > 1:
    m[rng.randrange(sq)] = False  # an all-False row: it sees the prefix only
  m[rng.randrange(sq), sq - 1] = True
  return m


# ----------------------------------------------------------------------------- the sweep's cases
SWEEP_SEEDS = tuple(range(40))
SWEEP_PAGES = (64, 128, 0)
SWEEP_HEADS = ((8, 2), (4, 4), (16, 4), (2, 1), (6, 2))
SWEEP_SPLITS = (0, 1, 3)


def draw_case(seed: int) -> dict:
  """The tree sweep's case of a seed, in ``kvcache_ref.draw_case``'s vocabulary (``kvcache_ref.materialize`` builds its tensors) plus ``mask_kind`` and
  ``per_sequence`` (a ``[B, Sq, Sq]`` mask).  Axis values are cycled over the seeds; lengths, Sq and the data are drawn from the seed's own generator."""
  rng = random.Random(seed * 6151 + 7)
  cls = R.PAGED_HEAD_DIM_CLASSES[(seed * 4) % 15]
  page = SWEEP_PAGES[seed % 3]
  unit = page or 64
  sq = (1, 2, 5, 64, 17, 33, 8, 63)[seed % 8] if seed % 5 else rng.randrange(1, 65)
  hq, hkv = SWEEP_HEADS[(seed // 3) % 5]
  B = 1 + (seed * 3) % 5
  reach = rng.randrange(2500, 5000) if seed % 7 == 3 else rng.randrange(80, 1200)
  pps = -(-reach // unit) + 1
  cap = pps * unit if page else reach + rng.randrange(0, 64)
  edges = (0, 1, sq - 1, sq, sq + 1, unit - 1, unit, unit + 1, cap)
  lens = [rng.choice(edges) if rng.random() < 0.25 else rng.randrange(1, cap) for _ in range(B)]
  c = dict(seed=seed, dtype=("bf16", "fp16")[(seed // 2) % 2], page=page, D=cls if seed % 4 else max(8, cls - 8 * rng.randrange(1, 7)), head_dim_class=cls,
           entry="plain", layout="separate", table_layout="plain", lens_strided=False, fused_qkv=False, heads=(hq, hkv), B=B,
           num_splits=SWEEP_SPLITS[(seed // 2) % 3], stream="auto", causal=False, return_lse=True, Sq=sq, Snew=None, rotary_dim=0, interleaved=True,
           pages_per_seq=pps, capacity=cap, seqlen_ro=cap, shared_prefix_len=0, lens=lens, bad_unused_ids=bool(page) and seed % 2 == 0, bad_used_id=False,
           share_prefix_pages=False, mask_kind=MASK_KINDS[seed % 5], per_sequence=seed % 3 == 1)
  return c


def case_mask(c: dict) -> torch.Tensor:
  """The mask of a drawn case (CPU): ``[Sq, Sq]``, or ``[B, Sq, Sq]`` with ``per_sequence``."""
  rng = random.Random(c["seed"] * 977 + 5)
  if c["per_sequence"]:
    return torch.stack([draw_mask(c["mask_kind"], c["Sq"], rng) for _ in range(c["B"])])
  return draw_mask(c["mask_kind"], c["Sq"], rng)


def visible_rows(c: dict) -> tuple:
  """``(query rows that see at least one key, query rows)`` per query head of a drawn case."""
  mask, sq = case_mask(c), c["Sq"]
  seen = 0
  for b, n in enumerate(R.effective_lens(c)):
    seen += int(visible(mask, b, n, sq).any(dim=1).sum()) if n > 0 else 0
  return seen, c["B"] * sq
